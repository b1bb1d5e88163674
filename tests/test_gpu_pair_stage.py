"""
GPU: pairs of views cut on the device (DeviceAugmenter.stage_pair: one launch of csrc/stage.hip over 2n rows) -- view by view
against the numpy restatement of the reference's transforms (oracle/augment.py), the mask mode of the ragged kernel against the
dense kernel (bit for bit on a uniform pool), the reference's own debugging check of a pair on the device's outputs
(tests/_pair_cases.compare_views), and the ICT / VAT / augmentation trainers end to end through their command lines on a
fabricated Pascal VOC tree (tests/_pascal_tree.py).

Bounds: those of tests/_stage_cases.py (image 2e-4, mask 1e-5, colour view 2e-3) and of tests/_pair_cases.py (1.5 grey levels).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden_json
import _pair_cases as pc
import _pascal_tree
import _stage_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = load_golden_json('pascal_source')


@pytest.fixture(scope='module')
def ragged():
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    images, labels = sc.make_pool_arrays()
    return ResidentPool(ArraySource(images, labels), range(len(images)), DEV, chunk_bytes=20000), images


def _augmenter(crop, aug_cfg, seed, cseed, dtype=torch.float32, mean=sc.MEAN, std=sc.STD):
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    return DeviceAugmenter(crop, mean, std, out_dtype=dtype, rng=np.random.RandomState(seed),
                           colour_rng=np.random.RandomState(cseed), **aug_cfg)


@pytest.mark.parametrize('name', list(pc.RAGGED))
def test_stage_pair_vs_numpy_oracle(ragged, name):
    pool, images = ragged
    crop, cfg, aug_cfg, seed, cseed = pc.RAGGED[name]
    n = len(sc.INDEX)
    aug = _augmenter(crop, aug_cfg, seed, cseed)
    params, xf01 = aug.draw_pair_params(pc.make_geometry(crop, cfg, seed), pool.sizes_of(sc.INDEX))
    assert params.shape == (2, n, 24) and xf01.shape == (n, 2, 3) and xf01.dtype == np.float32
    pc.assert_pair_branches_covered(cfg, params, crop)
    colour = bool(aug_cfg.get('strong_colour'))
    assert (params[0, :, 7:10] == 1).all() and not params[0, :, 10:15].any()              # view 0 carries no colour change
    if colour:
        assert set(params[1, :, 12].tolist()) == {0.0, 1.0} and params[1, :, 11].any()    # jitter applied and not; greyscale drawn
    else:
        assert (params[1, :, 7:10] == 1).all() and not params[1, :, 10:15].any()
    image0, image1, mask0, mask1, xf_got = aug.stage_pair(pool, sc.INDEX, None, drawn=(params, xf01))
    assert xf_got is xf01 and tuple(image0.shape) == tuple(image1.shape) == (n, 3) + tuple(crop)
    assert tuple(mask0.shape) == tuple(mask1.shape) == (n, 1) + tuple(crop) and mask0.dtype == torch.float32
    # the views of one batch are the halves of one buffer
    assert image1.data_ptr() == image0.data_ptr() + image0.numel() * image0.element_size()
    assert mask1.data_ptr() == mask0.data_ptr() + mask0.numel() * 4
    worst = [0.0, 0.0, 0.0]
    set_aside = total = 0
    for v, (img, msk) in enumerate(((image0, mask0), (image1, mask1))):
        img, msk = img.cpu().double().numpy(), msk[:, 0].cpu().double().numpy()
        for i, e in enumerate(sc.INDEX):
            p = params[v, i]
            pivot = sc.oracle_pivot(images[e], p, crop) if (colour and p[12]) else None
            w0, w1, wm = pc.oracle_view(images[e], p, crop, sc.MEAN, sc.STD, pivot=pivot)
            near = sc.near_rounding_boundary(p, crop)                                      # (no pair row rounds: bilinear / windows)
            keep = np.ones(crop, dtype=bool) if near is None else ~near
            set_aside += int((~keep).sum())
            total += keep.size
            tinted = v == 1 and colour
            want, tol, k = (w1, 2e-3, 2) if tinted else (w0, 2e-4, 0)
            worst[k] = max(worst[k], float(np.abs(img[i] - want)[:, keep].max()))
            worst[1] = max(worst[1], float(np.abs(msk[i] - wm)[keep].max()))
            np.testing.assert_allclose(img[i][:, keep], want[:, keep], rtol=tol, atol=tol, err_msg='image, view {} sample {}'.format(v, i))
            np.testing.assert_allclose(msk[i][keep], wm[keep], rtol=1e-5, atol=1e-5, err_msg='mask, view {} sample {}'.format(v, i))
    assert set_aside <= sc.MAX_BOUNDARY_FRACTION * total
    print('{}: largest differences image {:.3g}, mask {:.3g}, colour view {:.3g}'.format(name, *worst))
    if cfg.get('scale_hung'):
        assert set(torch.unique(mask1).tolist()) == {0.0, 1.0}                             # INTER_NEAREST of view 1's mask
    # drawing inside stage_pair() is the same draw
    again = _augmenter(crop, aug_cfg, seed, cseed).stage_pair(pool, sc.INDEX, pc.make_geometry(crop, cfg, seed))
    assert torch.equal(again[0], image0) and torch.equal(again[1], image1) and torch.equal(again[3], mask1)
    assert np.array_equal(again[4], xf01)


@pytest.mark.parametrize('geometry', ['window', 'warp'])
@pytest.mark.parametrize('colour', [False, True], ids=['plain', 'colour'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_uniform_pool_equals_the_dense_kernel_in_mask_mode_1(dtype, colour, geometry):
    """tests/test_gpu_stage.py's bit-for-bit property with slot 23 = 1 in all rows but one: both kernels call the one stage_mask;
    the images are those of slot 23 = 0."""
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    N, Hs, Ws = 6, 40, 70
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 256, (N, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 5, (N, Hs, Ws), generator=g).to(torch.uint8)
    pool = ResidentPool(ArraySource(list(src.numpy()), list(lab.numpy())), range(N), DEV)
    cfg = dict(scale_hung=True, hflip=True, vflip=True) if geometry == 'window' else dict(rot_mag=30.0, max_scale=1.5, hflip=True)
    aug = _augmenter((48, 64), dict(strong_colour=colour, **cfg), 11, 12, dtype=dtype)
    params = aug.draw_params(N, (Hs, Ws), with_labels=False)
    linear = aug.stage(pool, list(range(N)), True, params=params)
    params[:, 23] = 1.0
    params[int(np.argmin(params[:, 22])) if geometry == 'warp' else 2, 23] = 0.0       # one row (a nearest one of the warps) stays linear
    dense = aug(src.to(DEV), lab.to(DEV), params=params)
    got = aug.stage(pool, list(range(N)), True, params=params)
    assert set(got) == set(dense) and ('image_stu' in got) == colour
    for k in dense:
        assert got[k].dtype == dense[k].dtype and torch.equal(got[k], dense[k]), k
    on = torch.from_numpy(params[:, 23] != 0).to(DEV)
    assert set(torch.unique(got['mask'][on]).tolist()) == {0.0, 1.0}                       # the 40-row source is padded / left
    frac = (linear['mask'][on] > 0) & (linear['mask'][on] < 1)
    assert frac.any() and not torch.equal(got['mask'][on], linear['mask'][on])
    assert torch.equal(got['mask'][~on], linear['mask'][~on])
    assert torch.equal(got['image'], linear['image']) and torch.equal(got['labels'], linear['labels'])


@pytest.mark.parametrize('name', list(pc.SELF_CONSISTENCY))
def test_device_pairs_are_self_consistent(name):
    """The reference's debugging check (view 0 warped into view 1 agrees with view 1 where both masks are 1) on what stage_pair
    itself cut from a ramp source, fp32: tests/test_pair_stage_cpu.py's bound and its condition on the share compared."""
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    crop, src_hw, cfg = pc.SELF_CONSISTENCY[name]
    src = pc.ramp_source(src_hw)
    pool = ResidentPool(ArraySource([src], [np.zeros(src_hw, dtype=np.uint8)]), range(1), DEV)
    aug = _augmenter(crop, dict(), 0, 0, mean=None, std=None)
    image0, image1, mask0, mask1, xf01 = aug.stage_pair(pool, [0] * pc.N_PAIRS, pc.make_geometry(crop, cfg, pc.SEED))
    worst, share = pc.compare_views(image0, image1, mask0, mask1, xf01)
    print('{}: worst difference {:.2f} levels, smallest share compared {:.1%}'.format(name, worst.max(), share.min()))
    assert share.min() >= pc.MIN_COMPARED, share
    assert worst.max() <= pc.MAX_LEVELS, worst


TRAINER_RUNS = [('train_seg_semisup_ict', 'hung', ['--aug_scale_hung', '--aug_hflip', '--aug_strong_colour']),
                ('train_seg_semisup_vat_mt', 'hung', ['--aug_scale_hung', '--aug_hflip', '--aug_strong_colour']),
                ('train_seg_semisup_aug_mt', 'hung', ['--aug_scale_hung', '--aug_hflip', '--aug_strong_colour']),
                ('train_seg_semisup_aug_mt', 'warp', ['--aug_rot_mag', '30', '--aug_max_scale', '1.5'])]


@pytest.mark.parametrize('trainer_name,kind,aug_args', TRAINER_RUNS, ids=['{}-{}'.format(t[0][18:], t[1]) for t in TRAINER_RUNS])
def test_trainer_cli_on_a_fabricated_pascal_tree(trainer_name, kind, aug_args, tmp_path, monkeypatch):
    """The arguments of the CutMix trainer's test (tests/test_gpu_stage.py), plus --save_preds."""
    from click.testing import CliRunner
    trainer = __import__(trainer_name)
    tree = G['tree']
    train, val = tree['train'][:8], tree['val'][:4]
    sizes = {k: tree['sizes'][k] for k in train + val}
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), sizes, train, val)
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    base = ['--dataset', 'pascal', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2', '--crop_size', '65,65',
            '--n_sup', '4', '--num_epochs', '1', '--iters_per_epoch', '2', '--save_preds'] + aug_args
    for desc, extra in (('voc', []), ('voc_nval', ['--n_val', '2'])):
        res = CliRunner().invoke(trainer.experiment, ['--job_desc', desc] + base + extra, catch_exceptions=False)
        assert res.exit_code == 0, res.output
        out = tmp_path / 'results' / trainer_name
        log = open(out / 'log_{}.txt'.format(desc)).read()
        assert 'len(sup_ndx)=4' in log and 'Epoch 1' in log and 'img/s' not in log
        assert 'len(unsup_ndx)={}'.format(6 if extra else 8) in log and 'len(val_ndx)={}'.format(2 if extra else 4) in log
        m = re.search(r'Epoch 1: took [0-9.]+s, TRAIN clf loss=([0-9.naif-]+), consistency loss=([0-9.naif-]+), .*VAL mIoU=([0-9.naif-]+)%', log)
        assert m and all(math.isfinite(float(v)) for v in m.groups()), log
        assert ('FINAL TEST: mIoU=' in log) == bool(extra) and ('len(test_ndx)=4' in log) == bool(extra)
        # one prediction file per validation image, and per held-out test image (the reference writes both to the one place)
        preds = sorted(os.listdir(out / desc / 'preds'))
        assert len(preds) == (2 + 4 if extra else 4) and set(p + '.png' for p in val) <= set(preds), preds
