"""
GPU: CRF refinement (csrc/crf.hip through ops.crf_refine, crf.py, DatasetRun.staged_eval(crf=...), eval_seg --crf) against the fp64
restatement of tests/_crf_refs.py and the host-check driver, and end to end on the fabricated Pascal VOC tree and ISIC archive. Every
output is poisoned before the launch and sits between guard bytes that must survive it.
"""
import os
import re
import types

import numpy as np
import pytest
import torch

import _boundary_refs as BR
import _crf_refs as R
import _hostcheck
import _pascal_tree
import _zip_archives as Z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded(object):
    """A poisoned output tensor of `shape` inside a buffer with GUARD bytes of 0xA5 on both sides"""

    def __init__(self, shape, dtype, poison=0xFF):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + nbytes] = poison
        self.t = self.buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[-GUARD:] == 0xA5).all())


def params(inp, **over):
    return dict(dict(inp['prm'], radius=inp['radius'], dilation=inp['dilation'], iters=inp['iters']), **over)


def refine(inp, labels=True, want_q=True, rects=None, **over):
    """ops.crf_refine on a case's inputs with poisoned, guarded outputs -> dict(q, pred, stats, cm) on the host"""
    from cutmix_semisup_seg_amd import ops
    n, c = inp['logits'][0].shape[:2]
    H, W = inp['size']
    gp, gs = Guarded((n, H, W), torch.uint8), Guarded((2,), torch.int64)
    prm = params(inp, **{k: v for k, v in over.items() if k in R.PARAMS or k in ('radius', 'dilation', 'iters')})
    cm, pred, q, stats = ops.crf_refine([cu(l) for l in inp['logits']], inp['flips'], cu(inp['rgb']),
                                        inp['rects'] if rects is None else rects, c, (H, W), prm,
                                        labels=cu(inp['labels']) if labels else None, align_corners=inp['align'], pred=gp.t,
                                        want_q=want_q, stats_out=gs.t)
    torch.cuda.synchronize()
    assert gp.intact() and gs.intact() and pred is gp.t and stats is gs.t and (q is not None) == want_q
    return dict(q=None if q is None else q.cpu().numpy(), pred=pred.cpu().numpy(), stats=stats.cpu().numpy(),
                cm=None if cm is None else cm.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_kernel_vs_restatement_every_pixel(name):
    inp, ref = R.case(name)
    # conditions on the INPUTS, not tolerances: the reference decides every pixel by more than B can move Q
    assert ref['gap'] >= 4 * R.B and ref['unary_gap'] >= R.T.gap_bound(inp['k']) and ref['changed'] >= R.MIN_CHANGED
    got = refine(inp)
    print(name, 'max |Q - Q_fp64| on the GPU =', float(np.abs(got['q'] - ref['q']).max()), 'labels that differ:',
          int((got['pred'] != ref['pred']).sum()), 'changed', ref['changed'])
    R.compare(got, ref)
    assert np.array_equal(got['cm'], ref['cm'])
    assert np.isfinite(got['q']).all()


@pytest.fixture(scope='module')
def host():
    exe = _hostcheck.build('hostcheck_crf')
    return lambda inp: R.hostcheck_run(exe, inp)


@pytest.mark.parametrize('name', ['c5_r2s3_t5_k3', 'c21_r5s3_t5_k1', 'c64_r5s3_t1_k3', 'one_pixel'])
def test_kernel_vs_host_driver(host, name):
    """the same fp32 expressions in the same order; only expf, logf and the divisions may round otherwise"""
    inp, _ = R.case(name)
    got, want = refine(inp), host(inp)
    print(name, 'max |Q_gpu - Q_host| =', float(np.abs(got['q'] - want['q']).max()))
    assert np.abs(got['q'].astype(np.float64) - want['q']).max() <= R.B
    assert np.array_equal(got['pred'], want['pred']) and np.array_equal(got['stats'], want['stats'])


def test_one_and_five_iterations_from_the_same_buffers_and_repeated_calls():
    inp, ref5 = R.case('c5_r2s3_t5_k3')
    _, ref1 = R.case('c5_r2s3_t5_k3', iters=1)
    a5, a1, b5, b1 = refine(inp), refine(inp, iters=1), refine(inp), refine(inp, iters=1)
    for a, b in ((a5, b5), (a1, b1)):
        assert all(np.array_equal(a[k], b[k]) for k in ('q', 'pred', 'stats', 'cm'))      # the same bits
    assert np.abs(a1['q'] - ref1['q']).max() <= R.B and np.abs(a5['q'] - ref5['q']).max() <= R.B
    assert np.array_equal(a5['pred'], ref5['pred']) and not np.array_equal(a1['q'], a5['q'])
    # accumulation into a given matrix
    from cutmix_semisup_seg_amd import ops
    acc = cu(ref5['cm'].astype(np.int64))
    ops.crf_refine([cu(l) for l in inp['logits']], inp['flips'], cu(inp['rgb']), inp['rects'], inp['c'], inp['size'], params(inp),
                   labels=cu(inp['labels'].astype(np.int64)), align_corners=inp['align'], cm=acc)
    assert np.array_equal(acc.cpu().numpy(), 2 * ref5['cm'])


@pytest.mark.parametrize('name', ['c5_r2s3_t5_k3', 'c64_r5s3_t1_k3', 'c21_r5s16_t5_k3'])
def test_unary_argmax_is_the_vote_bit_for_bit(name):
    """outside the rectangles the prediction is the unary one: two calls with one-pixel rectangles elsewhere cover every pixel"""
    from cutmix_semisup_seg_amd import ops
    inp, _ = R.case(name)
    assert inp['k'] >= 2
    n, H, W = inp['shape']
    _, vote = ops.tta_vote([cu(l) for l in inp['logits']], inp['flips'], inp['c'], (H, W), align_corners=inp['align'], want_pred=True)
    vote = vote.cpu().numpy()
    a = refine(inp, labels=False, rects=np.array([[0, 0, 1, 1]] * n, dtype=np.int32))
    b = refine(inp, labels=False, rects=np.array([[H - 1, W - 1, 1, 1]] * n, dtype=np.int32))
    assert np.array_equal(a['pred'][:, 1:, :], vote[:, 1:, :]) and np.array_equal(a['pred'][:, :, 1:], vote[:, :, 1:])
    assert np.array_equal(b['pred'][:, 0, 0], vote[:, 0, 0])
    assert a['stats'].tolist() == [n, 0] and b['stats'].tolist() == [n, 0]           # a pixel without neighbours keeps its label


def test_sample_alone_equals_the_sample_in_its_batch_at_another_offset():
    """the same P and rgb: views of the canvas' own size are read without interpolation, so P moves with the pixels"""
    rng = np.random.RandomState(11)
    c, h, w = 21, 34, 49
    lg = np.clip(rng.standard_normal((c, h, w)) * 3.0, -8.0, 8.0).astype(np.float32)
    img = R.make_image(1, h, w, 11)[0]

    def placed(n, H, W, i, top, left):
        logits = np.clip(rng.standard_normal((n, c, H, W)) * 3.0, -8.0, 8.0).astype(np.float32)
        rgb = R.make_image(n, H, W, 12 + n)
        rects = np.array([[0, 0, H, W]] * n, dtype=np.int32)
        logits[i, :, top:top + h, left:left + w] = lg
        rgb[i, :, top:top + h, left:left + w] = img
        rects[i] = (top, left, h, w)
        inp = dict(logits=[logits], flips=[False], rgb=rgb, rects=rects, size=(H, W), align=True, radius=5, dilation=3, iters=5,
                   prm=dict(R.PARAMS, **R.STRONG), labels=None, shape=(n, H, W), c=c)
        got = refine(inp, labels=False)
        return got['q'][i, :, top:top + h, left:left + w], got['pred'][i, top:top + h, left:left + w]
    q_a, p_a = placed(2, 37, 53, 1, 3, 4)
    q_b, p_b = placed(1, 40, 60, 0, 5, 9)
    q_c, p_c = placed(3, 34, 49, 2, 0, 0)
    assert np.array_equal(q_a, q_b) and np.array_equal(p_a, p_b) and np.array_equal(q_a, q_c) and np.array_equal(p_a, p_c)
    assert len(np.unique(p_a)) > 1


def test_want_q_on_and_off_give_the_same_prediction():
    for name in ('c21_r5s3_t5_k1', 'c64_r2s3_t5_k1'):                                # one chunk of classes, two chunks
        inp, ref = R.case(name)
        on, off = refine(inp, want_q=True), refine(inp, want_q=False)
        assert np.array_equal(on['pred'], off['pred']) and np.array_equal(on['stats'], off['stats'])
        assert np.array_equal(on['cm'], off['cm']) and np.array_equal(on['pred'], ref['pred'])


def test_more_samples_than_one_launch_holds():
    """33 samples: the rectangles of 32 travel with one launch"""
    inp, ref = R.case('tiny_5x7')
    n = 33
    big = dict(inp, logits=[np.repeat(l, n, axis=0) for l in inp['logits']], rgb=np.repeat(inp['rgb'], n, axis=0),
               rects=np.repeat(inp['rects'], n, axis=0), labels=np.repeat(inp['labels'], n, axis=0), shape=(n, 5, 7))
    got = refine(big)
    assert all(np.array_equal(got['q'][i], got['q'][0]) and np.array_equal(got['pred'][i], got['pred'][0]) for i in range(n))
    assert np.array_equal(got['pred'][32], ref['pred'][0]) and np.array_equal(got['stats'], n * ref['stats'])
    assert np.array_equal(got['cm'], n * ref['cm'])


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZES = {'img_a': (40, 50), 'img_b': (44, 38), 'img_c': (36, 52), 'img_d': (41, 47), 'img_e': (40, 40)}
TRAIN, VAL = ['img_e'], ['img_a', 'img_b', 'img_c', 'img_d']


class _ColourNet(object):
    """stands in for a network: 21 classes whose logits are fixed mixtures of the standardised colour channels, at full resolution"""
    MEAN = STD = None
    BLOCK_SIZE = (8, 8)

    def forward_lowres(self, x):
        x = x.float()
        ang = torch.arange(21, dtype=torch.float32, device=x.device).view(1, 21, 1, 1)
        return (2.0 * (x[:, 0:1] * torch.cos(ang) + x[:, 1:2] * torch.sin(ang) + x[:, 2:3] * torch.cos(2.0 * ang))).contiguous()


def _crop(canvas_map, size):
    """an image of `size` out of the canvas it was centred on: dh // 2 rows above, dw // 2 columns to the left"""
    top, left = (canvas_map.shape[0] - size[0]) // 2, (canvas_map.shape[1] - size[1]) // 2
    return canvas_map[top:top + size[0], left:left + size[1]]


def _iou_lines(prefix, cm):
    diag = np.diag(cm).astype(float)
    iou = diag / np.maximum((cm.sum(axis=0) + cm.sum(axis=1)).astype(float) - diag, 1.0)
    return ['{} mIoU={:.3%}'.format(prefix, iou.mean()), '-- {}'.format(', '.join(['{:.3%}'.format(x) for x in iou]))]


def test_staged_eval_with_crf_on_the_pascal_tree(tmp_path, monkeypatch):
    from PIL import Image
    from cutmix_semisup_seg_amd import crf, evaluation, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets, seg_data
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), SIZES, TRAIN, VAL)
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    ds = datasets.load_dataset('pascal', -1, 131, -1, -1, 12345, None)
    net, src = _ColourNet(), ds['ds_src']
    run = tc.DatasetRun.for_evaluation(ds, ds['val_ndx_tgt'], net, torch.device(DEV), 3, torch.float32)
    step = types.SimpleNamespace(align_corners=True)
    # the canvas rgb equals the pool's bytes, from an fp32 augmenter and from a bf16 one (which stages once more in fp32)
    half = DeviceAugmenter((1, 1), run.augment.mean, run.augment.std, out_dtype=torch.bfloat16)
    assert np.abs(run.augment.mean).max() > 0 and np.abs(run.augment.std - 1).max() > 0
    for batch in seg_data.eval_batches(run.val_ndx, run.batch_size):
        ev = run.augment.stage_eval(run.pool, batch, net.BLOCK_SIZE)
        rects = crf.rects_of(ev['offsets'], run.pool.sizes_of(batch))
        for aug in (run.augment, half):
            rgb = crf.canvas_rgb(aug, run.pool, batch, net.BLOCK_SIZE)
            assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (len(batch), 3) + tuple(ev['canvas'])
            for k, i in enumerate(batch):
                top, left, h, w = rects[k]
                assert (h, w) == SIZES[src.sample_names[int(i)]]
                assert np.array_equal(rgb[k, :, top:top + h, left:left + w].cpu().numpy(), run.pool.image(int(i)).transpose(2, 0, 1))
    # the confusion matrix is the one of the saved files; the refinement does something
    prm = crf.CRFParams(iters=3)
    ev_crf, ev_plain = evaluation.EvaluatorIoU(21), evaluation.EvaluatorIoU(21)
    stats = run.staged_eval(net, step, run.val_ndx, ev_crf, str(tmp_path / 'crf'), crf=prm)
    assert run.staged_eval(net, step, run.val_ndx, ev_plain, str(tmp_path / 'plain')) is None
    want, changed, pixels = np.zeros((21, 21), dtype=np.int64), 0, 0
    for i in run.val_ndx:
        name = src.sample_names[int(i)] + '.png'
        t = run.pool.labels(int(i))
        p = _crop(np.asarray(Image.open(tmp_path / 'crf' / name)).astype(np.uint8), t.shape)
        want += R.T.confusion(t, p, 21)
        changed += int((p != _crop(np.asarray(Image.open(tmp_path / 'plain' / name)).astype(np.uint8), t.shape)).sum())
        pixels += t.size
    assert np.array_equal(ev_crf.cm, want.astype(np.float64)) and ev_crf.cm.sum() == ev_plain.cm.sum()
    assert stats.cpu().tolist() == [pixels, changed] and changed > 0
    print('pixels the refinement changes:', changed, 'of', pixels)


@pytest.fixture(scope='module')
def pascal(tmp_path_factory):
    """-> (working directory with the tree and its configuration, model.pth of a small DeepLab v2)"""
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    from oracle import deeplab2 as odl
    cwd = tmp_path_factory.mktemp('crf_pascal')
    root = _pascal_tree.write_tree(str(cwd / 'VOC2012'), SIZES, TRAIN, VAL)
    _pascal_tree.write_config(str(cwd), root)
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(21, [1, 1, 1, 1]))      # weights under which the classes are not tied
    model_path = str(cwd / 'model.pth')
    checkpoint.save_model(net, model_path)
    return cwd, root, model_path


def test_eval_seg_with_crf_end_to_end(pascal, monkeypatch, tmp_path):
    from click.testing import CliRunner
    from PIL import Image
    import eval_seg
    cwd, root, model_path = pascal
    monkeypatch.chdir(cwd)
    base = [model_path, '--dataset', 'pascal', '--batch_size', '3', '--compute_dtype', 'fp32', '--flip']
    res = CliRunner().invoke(eval_seg.experiment, base + ['--crf', '--crf_iters', '3', '--crf_bi_w', '40', '--crf_bi_rgb', '40',
                                                          '--crf_pos_w', '40', '--crf_pos_xy', '8', '--boundary_width', '2',
                                                          '--save_preds', str(tmp_path / 'crf')], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    plain = CliRunner().invoke(eval_seg.experiment, base + ['--save_preds', str(tmp_path / 'plain')], catch_exceptions=False)
    assert plain.exit_code == 0, plain.output
    cm, pairs, changed, pixels = np.zeros((21, 21), dtype=np.int64), [], 0, 0
    for name in VAL:
        t = np.asarray(Image.open(os.path.join(root, 'SegmentationClass', name + '.png')))
        p = _crop(np.asarray(Image.open(tmp_path / 'crf' / (name + '.png'))).astype(np.uint8), t.shape)
        cm += R.T.confusion(t, p, 21)
        pairs.append((t, p))
        changed += int((p != _crop(np.asarray(Image.open(tmp_path / 'plain' / (name + '.png'))).astype(np.uint8), t.shape)).sum())
        pixels += t.size
    want = _iou_lines('VAL', cm) + ['-- CRF changed {:.3%} of the pixels'.format(changed / pixels)]
    bcm, tcm = np.zeros((1, 22, 22), dtype=np.int64), np.zeros((1, 21, 21), dtype=np.int64)
    for t, p in pairs:
        b, tc = BR.confusion(t[None], p[None], 21, np.array([[2]]))
        bcm += b
        tcm += tc
    for tag, score in (('BIoU', BR.boundary_iou(bcm[0])), ('trimap', BR.plain_iou(tcm[0]))):
        want.append('VAL {}@2={:.3%}'.format(tag, score.mean()))
        want.append('-- {}@2 {}'.format(tag, ', '.join(['{:.3%}'.format(x) for x in score])))
    print('\n'.join(res.output.splitlines()[-7:]))
    assert res.output.splitlines()[-7:] == want
    # (that a refinement moves labels at all is test_staged_eval_with_crf_on_the_pascal_tree's to show: this network is sure of itself)
    print('pixels the refinement changes:', changed, 'of', pixels)


def test_lines_and_files_without_crf_are_unchanged(pascal, monkeypatch, tmp_path):
    from click.testing import CliRunner
    from PIL import Image
    from cutmix_semisup_seg_amd import checkpoint, evaluation, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets
    from cutmix_semisup_seg_amd.tta import TTA
    import eval_seg
    cwd, root, model_path = pascal
    monkeypatch.chdir(cwd)
    res = CliRunner().invoke(eval_seg.experiment, [model_path, '--dataset', 'pascal', '--batch_size', '2', '--compute_dtype', 'fp32',
                                                   '--scales', '0.75,1', '--save_preds', str(tmp_path / 'got')], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    ds = datasets.load_dataset('pascal', -1, 131, -1, -1, 12345, None)
    net = checkpoint.load_model(model_path).to(DEV)
    net.compute_dtype = torch.float32
    net.eval()
    run = tc.DatasetRun.for_evaluation(ds, ds['val_ndx_tgt'], net, torch.device(DEV), 2, torch.float32)
    ev = evaluation.EvaluatorIoU(21)
    tta = TTA((0.75, 1), False)
    # the path of the parent commit, spelled out: the vote counted by the evaluator, the plain vote saved
    os.makedirs(tmp_path / 'want')
    from cutmix_semisup_seg_amd.datapipe import seg_data
    with torch.no_grad():
        for batch in seg_data.eval_batches(run.val_ndx, 2):
            st = run.augment.stage_eval(run.pool, batch, net.BLOCK_SIZE)
            _, pred = tta.predict(net, st['image'], st['canvas'], net.upsample_align_corners, labels=st['labels'], want_pred=True,
                                  block_size=net.BLOCK_SIZE, evaluator=ev)
            for k, i in enumerate(batch):
                ds['ds_src'].save_prediction_by_index(str(tmp_path / 'want'), pred[k].cpu().numpy().astype(np.uint32), i)
    lines = [l for l in res.output.splitlines() if l.startswith('VAL') or l.startswith('-- ')]
    assert lines == _iou_lines('VAL', ev.cm) and 'CRF' not in res.output
    for n in VAL:
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'got' / (n + '.png'))), np.asarray(Image.open(tmp_path / 'want' / (n + '.png'))))


def test_bin_fill_holes_scores_the_filled_refined_map(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from PIL import Image
    from scipy import ndimage
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets
    from oracle import deeplab2 as odl
    import eval_seg
    Z.write_isic2017(str(tmp_path / 'isic2017.zip'))
    Z.write_config(str(tmp_path), isic2017=str(tmp_path / 'isic2017.zip'))
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 2, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(2, [1, 1, 1, 1]))
    model_path = str(tmp_path / 'model.pth')
    checkpoint.save_model(net, model_path)
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(eval_seg.experiment, [model_path, '--dataset', 'isic2017', '--batch_size', '3', '--compute_dtype', 'fp32',
                                                   '--bin_fill_holes', '--crf', '--crf_radius', '2', '--save_preds',
                                                   str(tmp_path / 'preds')], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    ds = datasets.load_dataset('isic2017', -1, 131, -1, -1, 12345, None)
    run_ = tc.DatasetRun.for_evaluation(ds, ds['val_ndx_tgt'], checkpoint.load_model(model_path).to(DEV), torch.device(DEV), 3,
                                        torch.float32)
    filled, plain, holes = np.zeros((2, 2), dtype=np.int64), np.zeros((2, 2), dtype=np.int64), 0
    for i in ds['val_ndx_tgt']:
        t = run_.pool.labels(int(i))
        saved = np.asarray(Image.open(tmp_path / 'preds' / (ds['ds_src'].sample_names[int(i)] + '.png')))
        p = (_crop(saved, t.shape) != 0).astype(np.uint8)                    # the file is the refined prediction, on its canvas
        f = _crop(ndimage.binary_fill_holes(saved != 0), t.shape).astype(np.uint8)      # filled as the evaluator fills it
        holes += int((f != p).sum())
        filled += R.T.confusion(t, f, 2)
        plain += R.T.confusion(t, p, 2)
    lines = [l for l in res.output.splitlines() if l.startswith('VAL') or l.startswith('-- ')]
    print('pixels the hole filling changes:', holes, lines)
    assert lines[:2] == _iou_lines('VAL', filled) and re.match(r'-- CRF changed \d+\.\d{3}% of the pixels$', lines[2])
    if holes:
        assert lines[:2] != _iou_lines('VAL', plain)


class _SpeckleNet(object):
    """stands in for a network: class 1 where the standardised red channel is positive, at full resolution. On the 4 x 4 blocks of
    noise of the fabricated images that is a foreground full of holes, which a weak refinement leaves in place."""
    MEAN = STD = None
    BLOCK_SIZE = (8, 8)

    def forward_lowres(self, x):
        r = x[:, 0:1].float()
        return torch.cat([-r, r], dim=1).contiguous()


def test_staged_eval_fills_the_holes_of_the_refined_map(tmp_path, monkeypatch):
    """with an IoU evaluator that fills holes the counts are the filled REFINED map's; the files stay the refined prediction"""
    from PIL import Image
    from scipy import ndimage
    from cutmix_semisup_seg_amd import crf, evaluation, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets
    Z.write_isic2017(str(tmp_path / 'isic2017.zip'))
    Z.write_config(str(tmp_path), isic2017=str(tmp_path / 'isic2017.zip'))
    monkeypatch.chdir(tmp_path)
    ds = datasets.load_dataset('isic2017', -1, 131, -1, -1, 12345, None)
    ndx, src, net = ds['val_ndx_tgt'], ds['ds_src'], _SpeckleNet()
    run_ = tc.DatasetRun.for_evaluation(ds, ndx, net, torch.device(DEV), 3, torch.float32)
    step = types.SimpleNamespace(align_corners=True)
    prm = crf.CRFParams(iters=2, radius=1, dilation=1, bi_w=0.5, pos_w=0.5)
    ev = evaluation.EvaluatorIoU(2, True)
    stats = run_.staged_eval(net, step, ndx, ev, str(tmp_path / 'crf'), crf=prm)
    run_.staged_eval(net, step, ndx, None, str(tmp_path / 'plain'))
    want, holes, changed = np.zeros((2, 2), dtype=np.int64), 0, 0
    for i in ndx:
        t = run_.pool.labels(int(i))
        name = src.sample_names[int(i)] + '.png'
        saved = np.asarray(Image.open(tmp_path / 'crf' / name))
        p = _crop(saved, t.shape).astype(np.uint8)
        f = _crop(ndimage.binary_fill_holes(saved != 0), t.shape).astype(np.uint8)
        holes += int((f != p).sum())
        changed += int((p != _crop(np.asarray(Image.open(tmp_path / 'plain' / name)), t.shape)).sum())
        want += R.T.confusion(t, f, 2)
    print('pixels the refinement changes:', changed, 'pixels the hole filling changes after it:', holes)
    assert np.array_equal(ev.cm, want.astype(np.float64))
    assert holes > 0 and changed > 0 and int(stats[1]) == changed
