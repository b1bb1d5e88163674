"""
GPU: the ragged staging path -- a pool of variable-sized images resident in HBM (resident_pool.py), gathered per batch sample by
csrc/stage.hip through DeviceAugmenter.stage / stage_eval -- against the numpy restatement of the reference's per-sample
transforms (oracle/augment.py), against the dense kernel (bit for bit on a uniform pool), against the reference's collate
geometry (tests/golden/pascal_source.json), and end to end through the CutMix trainer's command line on a fabricated Pascal VOC
tree (tests/_pascal_tree.py).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden_json
import _pascal_tree
import _stage_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = load_golden_json('pascal_source')


@pytest.fixture(scope='module')
def ragged():
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    images, labels = sc.make_pool_arrays()
    pool = ResidentPool(ArraySource(images, labels), range(len(images)), DEV, chunk_bytes=20000)
    return pool, images, labels


def test_pool_device_copy(ragged):
    pool, images, labels = ragged
    assert pool.image_buffer.is_cuda and pool.table_dev.is_cuda
    for i in range(len(images)):
        assert np.array_equal(pool.image(i), images[i]) and np.array_equal(pool.labels(i), labels[i])
        assert int(pool.table['img_off'][i]) % 16 == 0


@pytest.mark.parametrize('name', list(sc.CONFIGS))
def test_ragged_staging_vs_numpy_oracle(ragged, name):
    pool, images, labels = ragged
    aug, crop, with_labels, cfg = sc.make_augmenter(name)
    params = aug.draw_params(len(sc.INDEX), pool.sizes_of(sc.INDEX), with_labels=with_labels)
    sc.assert_branches_covered(name, params)
    res = aug.stage(pool, sc.INDEX, with_labels, params=params)
    assert ('labels' in res) == with_labels and ('image_stu' in res) == bool(cfg.get('strong_colour'))
    out = dict(image=res['image'].cpu().double().numpy(), mask=res['mask'][:, 0].cpu().double().numpy(),
               labels=res['labels'][:, 0].cpu().numpy() if with_labels else None,
               image_stu=res['image_stu'].cpu().double().numpy() if 'image_stu' in res else None)
    worst = sc.compare_with_oracle(name, params, images, labels, out)
    print('{}: largest differences image {:.3g}, mask {:.3g}, colour view {:.3g}'.format(name, *worst))
    if cfg.get('strong_colour'):
        same = [i for i in range(len(sc.INDEX)) if not params[i, 12] and not params[i, 11]]
        assert same and all(torch.equal(res['image'][i], res['image_stu'][i]) for i in same)
    # drawing inside stage() is the same draw
    aug2, _, _, _ = sc.make_augmenter(name)
    res2 = aug2.stage(pool, sc.INDEX, with_labels)
    assert torch.equal(res2['image'], res['image']) and torch.equal(res2['mask'], res['mask'])


@pytest.mark.parametrize('geometry', ['window', 'warp'])
@pytest.mark.parametrize('colour', [False, True], ids=['plain', 'colour'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_uniform_pool_equals_the_dense_kernel(dtype, colour, geometry):
    """A pool whose entries all have one size, index = arange: every output of the ragged kernel is the dense kernel's, bit for
    bit (same per-pixel functions, same luminance summation order)."""
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    N, Hs, Ws = 6, 60, 70
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 256, (N, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 5, (N, Hs, Ws), generator=g).to(torch.uint8)
    pool = ResidentPool(ArraySource(list(src.numpy()), list(lab.numpy())), range(N), DEV)
    cfg = dict(scale_hung=True, hflip=True, vflip=True) if geometry == 'window' else dict(rot_mag=30.0, max_scale=1.5, hflip=True)
    aug = DeviceAugmenter((48, 64), sc.MEAN, sc.STD, out_dtype=dtype, strong_colour=colour, rng=np.random.RandomState(11),
                          colour_rng=np.random.RandomState(12), **cfg)
    params = aug.draw_params(N, (Hs, Ws), with_labels=False)          # unlabelled draw: both interpolation modes of the warp
    if geometry == 'warp':
        assert set(params[:, 22].tolist()) == {0.0, 1.0}
    if colour:
        assert set(params[:, 12].tolist()) == {0.0, 1.0}
    dense = aug(src.to(DEV), lab.to(DEV), params=params)
    got = aug.stage(pool, list(range(N)), True, params=params)
    assert set(got) == set(dense) and ('image_stu' in got) == colour
    for k in dense:
        assert got[k].dtype == dense[k].dtype and torch.equal(got[k], dense[k]), k


@pytest.mark.parametrize('case', [c for c in G['collate'] if len(c['sizes']) == 3 and min(min(s) for s in c['sizes']) > 1],
                         ids=lambda c: 'block{}'.format(c['block_size'][0]))
def test_stage_eval_canvas(case):
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in case['sizes']]
    labels = [rng.randint(0, 21, size=(h, w)).astype(np.uint8) for h, w in case['sizes']]
    for l in labels:
        l[::7, ::5] = 255
    pool = ResidentPool(ArraySource(images, labels), range(len(images)), DEV)
    aug = DeviceAugmenter((33, 33), sc.MEAN, sc.STD, out_dtype=torch.float32)
    index = [2, 0, 1]
    ev = aug.stage_eval(pool, index, tuple(case['block_size']))
    assert list(ev['canvas']) == case['canvas'] and tuple(ev['image'].shape) == (3, 3) + tuple(case['canvas'])
    assert tuple(ev['labels'].shape) == (3, 1) + tuple(case['canvas']) and ev['labels'].dtype == torch.uint8
    img, lab = ev['image'].cpu().double().numpy(), ev['labels'][:, 0].cpu().numpy()
    for i, e in enumerate(index):
        h, w = case['sizes'][e]
        top, left = case['offsets'][e]                                  # the reference's SegCollate, whatever the batch order
        assert (top, left) == tuple(ev['offsets'][i])
        want = ((images[e].astype(np.float64) / 255.0 - sc.MEAN) / sc.STD).transpose(2, 0, 1)
        np.testing.assert_allclose(img[i][:, top:top + h, left:left + w], want, rtol=1e-5, atol=1e-5)
        assert np.array_equal(lab[i][top:top + h, left:left + w], labels[e])
        outside = np.ones(case['canvas'], dtype=bool)
        outside[top:top + h, left:left + w] = False
        assert (img[i][:, outside] == 0).all() and (lab[i][outside] == 255).all()


class _PixelNet(object):
    """A network whose prediction at a pixel is a fixed function of that input pixel alone (so it cannot depend on the canvas)"""

    def __init__(self, n_classes):
        g = torch.Generator().manual_seed(0)
        self.w = torch.randn(n_classes, 3, generator=g).to(DEV)
        self.b = torch.randn(n_classes, generator=g).to(DEV)

    def forward_lowres(self, x):
        return torch.einsum('ck,nkhw->nchw', self.w, x.float()) + self.b[None, :, None, None]


def test_padding_is_ignored_by_the_evaluation():
    """The EvaluatorIoU counts over a validation set staged in padded batches equal those of every image staged alone."""
    from cutmix_semisup_seg_amd import evaluation
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    from cutmix_semisup_seg_amd.datapipe import seg_data
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    C = 5
    sizes = [(70, 90), (93, 71), (75, 100), (100, 75), (81, 97)]
    rng = np.random.RandomState(1)
    images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    labels = [rng.randint(0, C, size=(h, w)).astype(np.uint8) for h, w in sizes]
    for l in labels:
        l[rng.uniform(size=l.shape) < 0.1] = 255
    pool = ResidentPool(ArraySource(images, labels), range(len(sizes)), DEV)
    aug = DeviceAugmenter((33, 33), sc.MEAN, sc.STD, out_dtype=torch.float32)
    net = _PixelNet(C)

    def counts(batch_size, block):
        ev_iou = evaluation.EvaluatorIoU(C)
        for b in seg_data.eval_batches(range(len(sizes)), batch_size):
            ev = aug.stage_eval(pool, b, block)
            ev_iou.sample_logits(net.forward_lowres(ev['image']), ev['labels'], ev['canvas'], ignore_value=255, align_corners=True)
        return ev_iou.cm
    alone = counts(1, (1, 1))
    assert alone.sum() == sum(int((l != 255).sum()) for l in labels)
    assert np.array_equal(counts(2, (1, 1)), alone) and np.array_equal(counts(3, (32, 32)), alone)
    assert np.array_equal(counts(5, (32, 32)), alone)


def test_trainer_cli_on_a_fabricated_pascal_tree(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_mask_mt as trainer
    tree = G['tree']
    train, val = tree['train'][:8], tree['val'][:4]
    sizes = {k: tree['sizes'][k] for k in train + val}
    assert all(70 <= h <= 120 and 70 <= w <= 120 for h, w in sizes.values()) and len({tuple(s) for s in sizes.values()}) > 4
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), sizes, train, val)
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    base = ['--dataset', 'pascal', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2', '--crop_size', '65,65',
            '--aug_scale_hung', '--aug_hflip', '--aug_strong_colour', '--n_sup', '4', '--num_epochs', '1', '--iters_per_epoch', '2']
    for desc, extra in (('voc', []), ('voc_nval', ['--n_val', '2'])):
        res = CliRunner().invoke(trainer.experiment, ['--job_desc', desc] + base + extra, catch_exceptions=False)
        assert res.exit_code == 0, res.output
        log = open(tmp_path / 'results' / 'train_seg_semisup_mask_mt' / 'log_{}.txt'.format(desc)).read()
        assert 'len(sup_ndx)=4' in log and 'Epoch 1' in log
        assert 'len(unsup_ndx)={}'.format(6 if extra else 8) in log and 'len(val_ndx)={}'.format(2 if extra else 4) in log
        m = re.search(r'VAL mIoU=([0-9.]+)%', log)
        assert m and math.isfinite(float(m.group(1)))
        assert ('FINAL TEST: mIoU=' in log) == bool(extra) and ('len(test_ndx)=4' in log) == bool(extra)
