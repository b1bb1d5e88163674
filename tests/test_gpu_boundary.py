"""
GPU: the boundary scores (csrc/boundary.hip through ops.boundary_confusion, evaluation.EvaluatorBoundary,
DatasetRun.staged_eval(boundary=...), eval_seg --boundary_width) against the scipy erosion reference of tests/_boundary_refs.py.
Everything is integer: every comparison is exact.
"""
import os
import re

import numpy as np
import pytest
import torch

import _boundary_refs as R
import _pascal_tree
import _zip_archives as Z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def cu(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # a copy: the shared cases are read-only


def run(truth, pred, c, widths, want_dist=True, **kw):
    """ops.boundary_confusion on host arrays -> dict of host arrays"""
    from cutmix_semisup_seg_amd import ops
    bcm, tcm, dist = ops.boundary_confusion(cu(truth), cu(pred), c, widths, want_dist=want_dist, **kw)
    torch.cuda.synchronize()
    out = dict(bcm=bcm.cpu().numpy(), tcm=tcm.cpu().numpy())
    if want_dist:
        out.update(dist_truth=dist[0].cpu().numpy(), dist_pred=dist[1].cpu().numpy())
    else:
        assert dist is None
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_matrices_and_distance_maps_vs_erosion_reference(name):
    inp, ref = R.case(name)
    got = run(inp['truth'], inp['pred'], inp['c'], inp['widths'])
    for key in ('dist_truth', 'dist_pred', 'bcm', 'tcm'):
        print(name, key, 'entries that differ:', int((got[key] != ref[key]).sum()))
    for key in ('dist_truth', 'dist_pred', 'bcm', 'tcm'):
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key
    # without the distance outputs: the same matrices
    again = run(inp['truth'], inp['pred'], inp['c'], inp['widths'], want_dist=False)
    assert np.array_equal(again['bcm'], ref['bcm']) and np.array_equal(again['tcm'], ref['tcm'])


def test_64_classes_one_width_per_counting_launch():
    truth, pred = R.blobs((2, 40, 50), 64, 11, sigma=1.0), R.blobs((2, 40, 50), 64, 12, sigma=1.0)
    widths = np.array([[1, 3, 2], [2, 2, 5]], dtype=np.int32)
    got = run(truth, pred, 64, widths, want_dist=False)
    bcm, tcm = R.confusion(truth, pred, 64, widths)
    assert np.array_equal(got['bcm'], bcm) and np.array_equal(got['tcm'], tcm)


def test_two_dimensional_maps_and_a_list_of_widths():
    inp, ref = R.case('c5_void')
    t, p = inp['truth'][0], inp['pred'][0]
    got = run(t, p, 5, [1, 2, 5, 254])
    bcm, tcm = R.confusion(t[None], p[None], 5, inp['widths'][:1])
    assert got['dist_truth'].shape == t.shape and np.array_equal(got['dist_truth'], ref['dist_truth'][0])
    assert np.array_equal(got['bcm'], bcm) and np.array_equal(got['tcm'], tcm)


def test_c_abi_null_outputs():
    """bcm alone, tcm alone, the distance maps alone (no widths): each accepted descriptor launches and writes what it was asked"""
    import ctypes
    from cutmix_semisup_seg_amd import _lib
    inp, ref = R.case('c5_void')
    t, p, w = cu(inp['truth']), cu(inp['pred']), cu(inp['widths'])
    n, h, wd = inp['truth'].shape
    need = _lib.fn['cms_boundary_workspace_bytes'](n, h, wd)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**out):
        d = _lib.BoundaryDesc()
        d.truth, d.pred, d.n, d.h, d.w, d.num_classes, d.ignore_index, d.k = t.data_ptr(), p.data_ptr(), n, h, wd, 5, 255, 4
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
        for key, val in out.items():
            setattr(d, key, val.data_ptr())
        _lib.check(_lib.fn['cms_boundary_confusion'](ctypes.byref(d), stream), 'cms_boundary_confusion')
        torch.cuda.synchronize()

    bcm = torch.zeros((4, 6, 6), dtype=torch.int64, device=DEV)
    tcm = torch.zeros((4, 5, 5), dtype=torch.int64, device=DEV)
    dt = torch.full((n, h, wd), 77, dtype=torch.uint8, device=DEV)
    call(bcm=bcm, widths=w)
    call(tcm=tcm, widths=w)
    call(dist_truth=dt)
    assert np.array_equal(bcm.cpu().numpy(), ref['bcm']) and np.array_equal(tcm.cpu().numpy(), ref['tcm'])
    assert np.array_equal(dt.cpu().numpy(), ref['dist_truth'])


# ------------------------------------------------------------------------------------------------------------------ independence
def _stacked():
    """Three images whose neighbours in memory continue each other: the last rows of one and the first rows of the next are the
    same constant class (and the last columns of a row and the first of the next row as well), so a window that crossed from one
    image -- or one row -- into the next would see no boundary where there is the array's edge."""
    truth = R.blobs((3, 33, 41), 5, 21).copy()
    pred = R.blobs((3, 33, 41), 5, 22, sigma=2.0).copy()
    for m, cl in ((truth, 2), (pred, 3)):
        m[:, :6] = cl
        m[:, -6:] = cl
    truth[1, 10:14, 20:30] = 255
    return truth, pred


def test_batch_of_three_is_the_sum_of_the_three_alone():
    truth, pred = _stacked()
    widths = np.array([[1, 3, 9, 40], [2, 3, 4, 5], [7, 1, 254, 2]], dtype=np.int32)
    whole = run(truth, pred, 5, widths)
    total_b, total_t = np.zeros_like(whole['bcm']), np.zeros_like(whole['tcm'])
    for i in range(3):
        one = run(truth[i:i + 1], pred[i:i + 1], 5, widths[i:i + 1])
        assert np.array_equal(one['dist_truth'][0], whole['dist_truth'][i]) and np.array_equal(one['dist_pred'][0], whole['dist_pred'][i])
        total_b += one['bcm']
        total_t += one['tcm']
    assert np.array_equal(total_b, whole['bcm']) and np.array_equal(total_t, whole['tcm'])
    # the first and last rows are the array's edge whatever lies beyond them in memory
    assert (whole['dist_truth'][:, 0] == 1).all() and (whole['dist_truth'][:, -1] == 1).all()
    assert (whole['dist_pred'][:, :, 0][truth[:, :, 0] != 255] == 1).all()
    bcm, tcm = R.confusion(truth, pred, 5, widths)
    assert np.array_equal(whole['bcm'], bcm) and np.array_equal(whole['tcm'], tcm)


@pytest.mark.parametrize('top,left,bottom,right', [(5, 7, 3, 11), (1, 1, 0, 0), (0, 0, 9, 67)])
def test_canvas_independence(top, left, bottom, right):
    """an image alone gives the matrices of the image centred (or not) on a larger canvas of 255"""
    inp, ref = R.case('c5_void')
    t, p = inp['truth'], inp['pred']
    n, h, w = t.shape
    big_t = np.full((n, h + top + bottom, w + left + right), 255, dtype=np.uint8)
    big_p = R.blobs(big_t.shape, 5, 31)                                 # what a network says on the padding is anything
    big_t[:, top:top + h, left:left + w] = t
    big_p[:, top:top + h, left:left + w] = p
    got = run(big_t, big_p, 5, inp['widths'])
    assert np.array_equal(got['bcm'], ref['bcm']) and np.array_equal(got['tcm'], ref['tcm'])
    assert np.array_equal(got['dist_truth'][:, top:top + h, left:left + w], ref['dist_truth'])
    assert np.array_equal(got['dist_pred'][:, top:top + h, left:left + w], ref['dist_pred'])
    inside = np.zeros(big_t.shape, dtype=bool)
    inside[:, top:top + h, left:left + w] = True
    assert (got['dist_truth'][~inside] == 0).all() and (got['dist_pred'][~inside] == 0).all()


def test_two_calls_into_the_same_matrices_double_them():
    from cutmix_semisup_seg_amd import ops
    inp, ref = R.case('c21_void')
    t, p = cu(inp['truth']), cu(inp['pred'])
    bcm, tcm, _ = ops.boundary_confusion(t, p, 21, inp['widths'])
    b2, t2, _ = ops.boundary_confusion(t, p, 21, inp['widths'], bcm=bcm, tcm=tcm)
    assert b2 is bcm and t2 is tcm
    assert np.array_equal(bcm.cpu().numpy(), 2 * ref['bcm']) and np.array_equal(tcm.cpu().numpy(), 2 * ref['tcm'])


@pytest.mark.parametrize('name', ['c2_k1', 'c5_void', 'c21_void'])
def test_identities(name):
    from cutmix_semisup_seg_amd import ops
    inp, ref = R.case(name)
    t, p, c = inp['truth'], inp['pred'], inp['c']
    n, h, w = t.shape
    big = max(h, w)
    assert big <= 254
    widths = np.array([[2, big]] * n, dtype=np.int32)
    got = run(t, p, c, widths)
    live = int((t != 255).sum())
    assert got['bcm'][0].sum() == live and got['bcm'][1].sum() == live                 # every non-void pixel, once per width
    for j, d in enumerate((2, big)):
        in_band = int(((got['dist_truth'] >= 1) & (got['dist_truth'] <= d)).sum())
        assert got['tcm'][j].sum() == in_band                                          # |B_T^d|
    # a band as wide as the image holds every pixel: the interior bin is empty and the rest is the plain confusion matrix
    cm = ops.confusion(cu(t), cu(p), c, ignore_index=255).cpu().numpy()
    assert not got['bcm'][1][c].any() and not got['bcm'][1][:, c].any()
    assert np.array_equal(got['bcm'][1][:c, :c], cm) and np.array_equal(got['tcm'][1], cm)


# ------------------------------------------------------------------------------------------------------------------ evaluator
def test_evaluator_with_ratio_widths_and_per_image_sizes():
    """three images of their own sizes, centred on one canvas as stage_eval pads them; a ratio refers to each image's own diagonal"""
    from cutmix_semisup_seg_amd import evaluation
    sizes = [(33, 41), (60, 25), (48, 64)]
    spec = [2, 0.05, 0.2]
    canvas = (65, 65)
    truth = np.full((3,) + canvas, 255, dtype=np.uint8)
    pred = R.blobs((3,) + canvas, 5, 41)
    want_b, want_t = np.zeros((3, 6, 6), dtype=np.int64), np.zeros((3, 5, 5), dtype=np.int64)
    px = []
    for i, (h, w) in enumerate(sizes):
        top, left = (canvas[0] - h) // 2, (canvas[1] - w) // 2
        t = R.with_void(R.blobs((1, h, w), 5, 50 + i), 60 + i)
        truth[i, top:top + h, left:left + w] = t[0]
        widths = [R.width_px(s, (h, w)) for s in spec]
        px.append(widths)
        b, tc = R.confusion(t, pred[i:i + 1, top:top + h, left:left + w], 5, np.array([widths]))
        want_b += b
        want_t += tc
    assert px == [[2, 3, 11], [2, 3, 13], [2, 4, 16]]                       # the diagonals are 52.6, 65 and 80
    ev = evaluation.EvaluatorBoundary(5, spec)
    ev.sample(cu(truth), cu(pred), sizes=sizes)
    assert np.array_equal(ev.bcm, want_b) and np.array_equal(ev.tcm, want_t)
    assert np.array_equal(ev.boundary_iou(), R.boundary_iou(want_b)) and ev.boundary_iou().shape == (3, 5)
    assert np.array_equal(ev.trimap_iou(), R.plain_iou(want_t)) and ev.trimap_iou().shape == (3, 5)
    # a second sample accumulates; numpy maps and a 2-D pair are taken; without sizes the map's own size is the image
    ev.sample(truth[0], pred[0])
    b, tc = R.confusion(truth[:1], pred[:1], 5, np.array([[R.width_px(s, canvas) for s in spec]]))
    assert np.array_equal(ev.bcm, want_b + b) and np.array_equal(ev.tcm, want_t + tc)
    with pytest.raises(ValueError):
        ev.sample(cu(truth), cu(pred), sizes=sizes[:2])


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZES = {'img_a': (40, 50), 'img_b': (44, 38), 'img_c': (36, 52), 'img_d': (41, 47), 'img_e': (40, 40)}
TRAIN, VAL = ['img_e'], ['img_a', 'img_b', 'img_c', 'img_d']


def _score_lines(prefix, labels_and_preds, c, spec):
    """the lines eval_seg prints after its two, from per-image (truth, prediction) pairs by the reference"""
    k = len(spec)
    bcm, tcm = np.zeros((k, c + 1, c + 1), dtype=np.int64), np.zeros((k, c, c), dtype=np.int64)
    for t, p in labels_and_preds:
        b, tc = R.confusion(t[None], p[None], c, np.array([[R.width_px(s, t.shape) for _, s in spec]]))
        bcm += b
        tcm += tc
    lines = []
    for j, (label, _) in enumerate(spec):
        for name, score in (('BIoU', R.boundary_iou(bcm[j])), ('trimap', R.plain_iou(tcm[j]))):
            lines.append('{} {}@{}={:.3%}'.format(prefix, name, label, score.mean()))
            lines.append('-- {}@{} {}'.format(name, label, ', '.join(['{:.3%}'.format(x) for x in score])))
    return lines, bcm


def _crop(canvas_map, size):
    """an image of `size` out of the canvas it was centred on: dh // 2 rows above, dw // 2 columns to the left"""
    top, left = (canvas_map.shape[0] - size[0]) // 2, (canvas_map.shape[1] - size[1]) // 2
    return canvas_map[top:top + size[0], left:left + size[1]]


def test_eval_seg_end_to_end_on_pascal(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from PIL import Image
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    from oracle import deeplab2 as odl
    import eval_seg
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), SIZES, TRAIN, VAL)
    _pascal_tree.write_config(str(tmp_path), root)
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(21, [1, 1, 1, 1]))
    model_path = str(tmp_path / 'model.pth')
    checkpoint.save_model(net, model_path)
    monkeypatch.chdir(tmp_path)

    def picked(output, pattern):
        return [l for l in output.splitlines() if re.match(pattern, l)]
    two = r'VAL mIoU=|-- (?!BIoU@|trimap@)'
    assert [R.width_px(0.05, SIZES[n]) for n in VAL] == [3, 3, 3, 3]                # diagonals of 58 to 64 pixels
    # the vote over a view and its mirror image, and the single view
    for tag, extra in (('flip', ['--flip']), ('single', [])):
        base = [model_path, '--dataset', 'pascal', '--batch_size', '3', '--compute_dtype', 'fp32'] + extra
        res = CliRunner().invoke(eval_seg.experiment, base + ['--boundary_width', '2,0.05', '--save_preds', str(tmp_path / tag)],
                                 catch_exceptions=False)
        assert res.exit_code == 0, res.output
        plain = CliRunner().invoke(eval_seg.experiment, base, catch_exceptions=False)
        assert plain.exit_code == 0, plain.output
        assert len(picked(plain.output, two)) == 2 and picked(res.output, two) == picked(plain.output, two)
        assert not picked(plain.output, r'.*(BIoU|trimap)')
        pairs = []
        for name in VAL:
            t = np.asarray(Image.open(os.path.join(root, 'SegmentationClass', name + '.png')))
            assert t.shape == SIZES[name] and t.dtype == np.uint8 and (t == 255).any()
            pairs.append((t, _crop(np.asarray(Image.open(tmp_path / tag / (name + '.png'))).astype(np.uint8), t.shape)))
        want, bcm = _score_lines('VAL', pairs, 21, [('2', 2), ('0.05', 0.05)])
        got = picked(res.output, r'VAL (BIoU|trimap)@|-- (BIoU|trimap)@')
        print(tag, 'classes predicted inside the images:', sorted(set(int(v) for _, p in pairs for v in np.unique(p))))
        print('\n'.join(got))
        assert got == want
        assert bcm.sum() == 2 * sum(int((t != 255).sum()) for t, _ in pairs)
        # the lines come after the two, in the spec's order
        assert res.output.splitlines()[-8:] == want and res.output.splitlines()[-10].startswith('VAL mIoU=')


def test_eval_seg_with_bin_fill_holes_scores_the_filled_map(tmp_path, monkeypatch):
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
                                                   '--bin_fill_holes', '--boundary_width', '3', '--save_preds', str(tmp_path / 'preds')],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    # the labels as the evaluation sees them: the pool's, un-padded
    ds = datasets.load_dataset('isic2017', -1, 131, -1, -1, 12345, None)
    run_ = tc.DatasetRun.for_evaluation(ds, ds['val_ndx_tgt'], checkpoint.load_model(model_path).to(DEV), torch.device(DEV), 3,
                                        torch.float32)
    src = ds['ds_src']
    filled, plain, holes = [], [], 0
    for i in ds['val_ndx_tgt']:
        t = run_.pool.labels(int(i))
        saved = np.asarray(Image.open(tmp_path / 'preds' / (src.sample_names[int(i)] + '.png')))
        p = (_crop(saved, t.shape) != 0).astype(np.uint8)                    # the file is the plain prediction, on its canvas
        # filled as the mIoU line's evaluator fills it: the batch's canvas map, padding included, then the image cut out
        f = _crop(ndimage.binary_fill_holes(saved != 0), t.shape).astype(np.uint8)
        holes += int((f != p).sum())
        filled.append((t, f))
        plain.append((t, p))
    want, _ = _score_lines('VAL', filled, 2, [('3', 3)])
    got = [l for l in res.output.splitlines() if 'BIoU@' in l or 'trimap@' in l]
    print('pixels the hole filling changes:', holes)
    print('\n'.join(got))
    assert got == want
    if holes:
        assert got != _score_lines('VAL', plain, 2, [('3', 3)])[0]


class _SpeckleNet(object):
    """stands in for a network: class 1 where the standardised red channel is positive, at full resolution. On the 4 x 4 blocks of
    noise of the fabricated images that is a foreground full of holes."""
    MEAN = STD = None
    BLOCK_SIZE = (8, 8)

    def forward_lowres(self, x):
        r = x[:, 0:1].float()
        return torch.cat([-r, r], dim=1).contiguous()


def test_staged_eval_fills_holes_before_scoring(tmp_path, monkeypatch):
    """with an IoU evaluator that fills holes the boundary scores are the filled map's; the files stay the plain prediction"""
    import types
    from PIL import Image
    from scipy import ndimage
    from cutmix_semisup_seg_amd import evaluation, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets
    Z.write_isic2017(str(tmp_path / 'isic2017.zip'))
    Z.write_config(str(tmp_path), isic2017=str(tmp_path / 'isic2017.zip'))
    monkeypatch.chdir(tmp_path)
    ds = datasets.load_dataset('isic2017', -1, 131, -1, -1, 12345, None)
    ndx, src, net, spec = ds['val_ndx_tgt'], ds['ds_src'], _SpeckleNet(), [3, 0.05]
    run_ = tc.DatasetRun.for_evaluation(ds, ndx, net, torch.device(DEV), 3, torch.float32)
    step = types.SimpleNamespace(align_corners=True)
    got = {}
    for tag, fill in (('filled', True), ('plain', False)):
        bd = evaluation.EvaluatorBoundary(2, spec)
        run_.staged_eval(net, step, ndx, evaluation.EvaluatorIoU(2, fill), str(tmp_path / tag), boundary=bd)
        got[tag] = (bd.bcm, bd.tcm)
    want = {tag: [np.zeros((2, 3, 3), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64)] for tag in got}
    holes = 0
    for i in ndx:
        t = run_.pool.labels(int(i))
        name = src.sample_names[int(i)] + '.png'
        saved = np.asarray(Image.open(tmp_path / 'filled' / name))
        assert np.array_equal(saved, np.asarray(Image.open(tmp_path / 'plain' / name)))          # the plain prediction both times
        widths = np.array([[R.width_px(s, t.shape) for s in spec]])
        maps = dict(plain=_crop(saved, t.shape).astype(np.uint8),
                    filled=_crop(ndimage.binary_fill_holes(saved != 0), t.shape).astype(np.uint8))
        holes += int((maps['plain'] != maps['filled']).sum())
        for tag, p in maps.items():
            b, tc_ = R.confusion(t[None], p[None], 2, widths)
            want[tag][0] += b
            want[tag][1] += tc_
    print('pixels the hole filling changes:', holes)
    assert holes > 0
    for tag in got:
        assert np.array_equal(got[tag][0], want[tag][0]) and np.array_equal(got[tag][1], want[tag][1]), tag
    assert not np.array_equal(got['filled'][0], got['plain'][0])
