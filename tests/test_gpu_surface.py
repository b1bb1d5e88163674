"""
GPU: the surface distances (csrc/surface.hip through ops.surface_distances, evaluation.EvaluatorSurface,
DatasetRun.staged_eval(surface=...), eval_seg --surface_dist) against the scipy reference of tests/_surface_refs.py. The integers
(`stats`, the two d2 maps) are compared exactly; the fp64 sums within relative (n + 2) 2^-52, n the surface pixels summed: the worst
case of adding n square roots that are correctly rounded or one ulp off, in any order.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _pascal_tree
import _surface_refs as R
import _zip_archives as Z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def cu(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # a copy: the shared cases are read-only


def run(truth, pred, c, want_maps=True, **kw):
    """ops.surface_distances on host arrays -> dict of host arrays"""
    from cutmix_semisup_seg_amd import ops
    stats, sums, maps = ops.surface_distances(cu(truth), cu(pred), c, want_maps=want_maps, **kw)
    torch.cuda.synchronize()
    out = dict(stats=stats.cpu().numpy(), sums=sums.cpu().numpy())
    if want_maps:
        out.update(d2_pred=maps[0].cpu().numpy(), d2_truth=maps[1].cpu().numpy())
    else:
        assert maps is None
    return out


def _same(got, ref, what=''):
    keys = [k for k in ('stats', 'd2_pred', 'd2_truth') if k in got]
    for key in keys:
        print(what, key, 'entries that differ:', int((got[key] != ref[key]).sum()))
    for key in keys:
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key
    assert got['sums'].dtype == np.float64 and R.sums_close(got['sums'], ref['sums'], ref['stats'])


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_stats_sums_and_maps_vs_scipy_reference(name):
    inp, ref = R.case(name)
    got = run(inp['truth'], inp['pred'], inp['c'])
    _same(got, ref, name)
    # a second call: the same bits, the sums included; and without the maps the same numbers
    again = run(inp['truth'], inp['pred'], inp['c'])
    assert again['sums'].tobytes() == got['sums'].tobytes() and np.array_equal(again['stats'], got['stats'])
    bare = run(inp['truth'], inp['pred'], inp['c'], want_maps=False)
    assert bare['sums'].tobytes() == got['sums'].tobytes() and np.array_equal(bare['stats'], got['stats'])


def test_two_dimensional_maps_and_no_ignore_index():
    inp, ref = R.case('c5_void')
    t, p = inp['truth'][1], inp['pred'][1]
    got = run(t, p, 5)
    assert got['d2_pred'].shape == t.shape and got['stats'].shape == (1, 5, 6)
    assert np.array_equal(got['stats'][0], ref['stats'][1]) and np.array_equal(got['d2_truth'], ref['d2_truth'][1])
    # without an ignore index 255 is a value like any other: no class, outside every mask
    _same(run(inp['truth'], inp['pred'], 5, ignore_index=None), R.reference(inp['truth'], inp['pred'], 5, ignore=None))


def test_c_abi_null_outputs():
    """the maps NULL, stats alone, sums alone, one map alone: each accepted descriptor launches and writes what it was asked"""
    from cutmix_semisup_seg_amd import _lib
    inp, ref = R.case('c21_void')
    t, p = cu(inp['truth']), cu(inp['pred'])
    n, h, w = inp['truth'].shape
    need = _lib.fn['cms_surface_workspace_bytes'](n, h, w, 21)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**out):
        d = _lib.SurfaceDesc()
        d.truth, d.pred, d.n, d.h, d.w, d.num_classes, d.ignore_index = t.data_ptr(), p.data_ptr(), n, h, w, 21, 255
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
        for key, val in out.items():
            setattr(d, key, val.data_ptr())
        _lib.check(_lib.fn['cms_surface_distances'](ctypes.byref(d), stream), 'cms_surface_distances')
        torch.cuda.synchronize()

    def fresh():
        return (torch.full((n, 21, 6), 77, dtype=torch.int64, device=DEV), torch.full((n, 21, 2), 7.0, dtype=torch.float64, device=DEV),
                torch.full((n, h, w), 77, dtype=torch.int32, device=DEV))
    stats, sums, _ = fresh()
    call(stats=stats, sums=sums)
    _same(dict(stats=stats.cpu().numpy(), sums=sums.cpu().numpy()), ref)
    stats, sums, d2 = fresh()
    call(stats=stats)
    assert np.array_equal(stats.cpu().numpy(), ref['stats']) and (sums == 7.0).all()
    stats, sums, d2 = fresh()
    call(sums=sums)
    assert R.sums_close(sums.cpu().numpy(), ref['sums'], ref['stats']) and (stats == 77).all()
    call(d2_truth=d2)
    assert np.array_equal(d2.cpu().numpy(), ref['d2_truth']) and (stats == 77).all()


# ------------------------------------------------------------------------------------------------------------------ independence
def _stacked():
    """Three images whose neighbours in memory continue each other: the last rows of one and the first rows of the next are the
    same constant class (and the last columns of a row and the first of the next row as well), so a walk that crossed from one
    image -- or one row -- into the next would see no surface where there is the array's edge, and a nearer pixel where there is
    none."""
    truth = R.blobs((3, 33, 41), 5, 21).copy()
    pred = R.blobs((3, 33, 41), 5, 22, sigma=2.0).copy()
    for m, cl in ((truth, 2), (pred, 3)):
        m[:, :6] = cl
        m[:, -6:] = cl
    truth[1, 10:14, 20:30] = 255
    return truth, pred


def test_batch_of_three_is_the_three_alone():
    truth, pred = _stacked()
    whole = run(truth, pred, 5)
    for i in range(3):
        one = run(truth[i:i + 1], pred[i:i + 1], 5)
        for key in ('stats', 'd2_pred', 'd2_truth'):
            assert np.array_equal(one[key][0], whole[key][i]), (key, i)
        assert one['sums'].tobytes() == whole['sums'][i:i + 1].tobytes()
    _same(whole, R.reference(truth, pred, 5), 'stacked')
    # the first and last rows are the array's edge whatever lies beyond them in memory: surface pixels of the truth
    assert (whole['d2_truth'][:, 0] >= 0).all() and (whole['d2_truth'][:, -1] >= 0).all()


@pytest.mark.parametrize('top,left,bottom,right', [(5, 7, 3, 11), (1, 1, 0, 0), (0, 0, 9, 67)])
def test_canvas_independence(top, left, bottom, right):
    """an image alone gives the numbers of the image anywhere on a larger canvas of 255, whatever the prediction says there"""
    inp, ref = R.case('c5_void')
    t, p = inp['truth'], inp['pred']
    n, h, w = t.shape
    big_t = np.full((n, h + top + bottom, w + left + right), 255, dtype=np.uint8)
    big_p = R.blobs(big_t.shape, 5, 31)
    big_t[:, top:top + h, left:left + w] = t
    big_p[:, top:top + h, left:left + w] = p
    got = run(big_t, big_p, 5)
    assert np.array_equal(got['stats'], ref['stats']) and R.sums_close(got['sums'], ref['sums'], ref['stats'])
    assert np.array_equal(got['d2_pred'][:, top:top + h, left:left + w], ref['d2_pred'])
    assert np.array_equal(got['d2_truth'][:, top:top + h, left:left + w], ref['d2_truth'])
    inside = np.zeros(big_t.shape, dtype=bool)
    inside[:, top:top + h, left:left + w] = True
    assert (got['d2_pred'][~inside] == -1).all() and (got['d2_truth'][~inside] == -1).all()


# ------------------------------------------------------------------------------------------------------------------ evaluator
def _close(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all(), (got, want)


def test_evaluator_over_images_of_their_own_sizes():
    """three images centred on one canvas as stage_eval pads them, then a second batch; class 5 is in no map"""
    from cutmix_semisup_seg_amd import evaluation
    sizes, canvas = [(33, 41), (60, 25), (48, 64)], (65, 65)
    truth = np.full((3,) + canvas, 255, dtype=np.uint8)
    pred = R.blobs((3,) + canvas, 5, 41)
    refs = []
    for i, (h, w) in enumerate(sizes):
        top, left = (canvas[0] - h) // 2, (canvas[1] - w) // 2
        t = R.with_void(R.blobs((1, h, w), 5, 50 + i), 60 + i)
        truth[i, top:top + h, left:left + w] = t[0]
        refs.append(R.reference(t, pred[i:i + 1, top:top + h, left:left + w], 6))
    ev = evaluation.EvaluatorSurface(6)
    ev.sample(cu(truth), cu(pred))
    want = R.dataset(refs)
    assert want['scored'][:5].min() >= 2 and want['scored'][5] == 0
    for got, key in ((ev.hd(), 'hd'), (ev.hd95(), 'hd95'), (ev.assd(), 'assd')):
        _close(got, want[key])
    assert np.isnan(ev.hd95()[5]) and not np.isnan(ev.hd95()[:5]).any()
    scored, one_sided = ev.pairs()
    assert scored.dtype == np.int64 and np.array_equal(scored, want['scored']) and np.array_equal(one_sided, want['one_sided'])
    # a second sample accumulates; numpy maps and a 2-D pair are taken
    inp, ref = R.case('one_sided')
    ev.sample(np.array(inp['truth'][1]), np.array(inp['pred'][1]))
    more = R.reference(inp['truth'][1:], inp['pred'][1:], 6)
    want = R.dataset(refs + [more])
    assert want['one_sided'].sum() >= 2
    for got, key in ((ev.hd(), 'hd'), (ev.hd95(), 'hd95'), (ev.assd(), 'assd')):
        _close(got, want[key])
    assert [a.tolist() for a in ev.pairs()] == [want['scored'].tolist(), want['one_sided'].tolist()]
    assert abs(evaluation.EvaluatorSurface.headline(ev.hd95()) - np.nanmean(want['hd95'])) <= 1e-12 * np.nanmean(want['hd95'])


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZES = {'img_a': (40, 50), 'img_b': (44, 38), 'img_c': (36, 52), 'img_d': (41, 47), 'img_e': (40, 40)}
TRAIN, VAL = ['img_e'], ['img_a', 'img_b', 'img_c', 'img_d']
NEW = r'(VAL|TEST) (HD95|ASSD|HD)=|-- (HD95|ASSD|HD|surface pairs) '


def _crop(canvas_map, size):
    """an image of `size` out of the canvas it was centred on: dh // 2 rows above, dw // 2 columns to the left"""
    top, left = (canvas_map.shape[0] - size[0]) // 2, (canvas_map.shape[1] - size[1]) // 2
    return canvas_map[top:top + size[0], left:left + size[1]]


def _lines(prefix, labels_and_preds, c):
    return R.lines(prefix, R.dataset([R.reference(t[None], p[None], c) for t, p in labels_and_preds]))


def _split(output):
    lines = output.splitlines()
    return [l for l in lines if not re.match(NEW, l)], [l for l in lines if re.match(NEW, l)]


@pytest.fixture(scope='module')
def pascal(tmp_path_factory):
    """-> (working directory with the tree and its configuration, the tree, model.pth of a small closed-form DeepLab v2)"""
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    from oracle import deeplab2 as odl
    cwd = tmp_path_factory.mktemp('surface_pascal')
    root = _pascal_tree.write_tree(str(cwd / 'VOC2012'), SIZES, TRAIN, VAL)
    _pascal_tree.write_config(str(cwd), root)
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(21, [1, 1, 1, 1]))
    model_path = str(cwd / 'model.pth')
    checkpoint.save_model(net, model_path)
    return cwd, root, model_path


def _pascal_pairs(root, preds_dir):
    from PIL import Image
    pairs = []
    for name in VAL:
        t = np.asarray(Image.open(os.path.join(root, 'SegmentationClass', name + '.png')))
        assert t.shape == SIZES[name] and t.dtype == np.uint8 and (t == 255).any()
        pairs.append((t, _crop(np.asarray(Image.open(os.path.join(preds_dir, name + '.png'))).astype(np.uint8), t.shape)))
    return pairs


@pytest.mark.parametrize('extra', [[], ['--crf', '--crf_iters', '3', '--crf_bi_w', '40', '--crf_bi_rgb', '40', '--crf_pos_w', '40',
                                        '--crf_pos_xy', '8', '--boundary_width', '2']], ids=['plain', 'crf'])
def test_eval_seg_end_to_end_on_pascal(pascal, monkeypatch, tmp_path, extra):
    """the seven lines are those of the saved files -- the refined ones with --crf -- and every line before them is unchanged"""
    from click.testing import CliRunner
    import eval_seg
    cwd, root, model_path = pascal
    monkeypatch.chdir(cwd)
    base = [model_path, '--dataset', 'pascal', '--batch_size', '3', '--compute_dtype', 'fp32'] + extra
    res = CliRunner().invoke(eval_seg.experiment, base + ['--surface_dist', '--save_preds', str(tmp_path / 'with')],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    plain = CliRunner().invoke(eval_seg.experiment, base + ['--save_preds', str(tmp_path / 'without')], catch_exceptions=False)
    assert plain.exit_code == 0, plain.output
    old, new = _split(res.output)
    assert _split(plain.output) == (old, []) and len(old) >= 2
    pairs = _pascal_pairs(root, str(tmp_path / 'with'))
    for (_, a), (_, b) in zip(pairs, _pascal_pairs(root, str(tmp_path / 'without'))):
        assert np.array_equal(a, b)                                         # the files do not depend on the option
    want = _lines('VAL', pairs, 21)
    print('\n'.join(new))
    assert new == want and res.output.splitlines()[-7:] == want
    assert re.match(r'VAL HD95=\d+\.\d{3}$', new[0]) and ' -' in new[1] and re.search(r'\d+\.\d{3}', new[1])


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
                                                   '--bin_fill_holes', '--surface_dist', '--save_preds', str(tmp_path / 'preds')],
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
    want = _lines('VAL', filled, 2)
    got = _split(res.output)[1]
    print('pixels the hole filling changes:', holes)
    print('\n'.join(got))
    assert got == want
    if holes:
        assert got != _lines('VAL', plain, 2)


class _SpeckleNet(object):
    """stands in for a network: class 1 where the standardised red channel is positive, at full resolution. On the 4 x 4 blocks of
    noise of the fabricated images that is a foreground full of holes."""
    MEAN = STD = None
    BLOCK_SIZE = (8, 8)

    def forward_lowres(self, x):
        r = x[:, 0:1].float()
        return torch.cat([-r, r], dim=1).contiguous()


def test_staged_eval_fills_holes_before_scoring(tmp_path, monkeypatch):
    """with an IoU evaluator that fills holes the surface distances are the filled map's; the files stay the plain prediction"""
    import types
    from PIL import Image
    from scipy import ndimage
    from cutmix_semisup_seg_amd import evaluation, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets
    Z.write_isic2017(str(tmp_path / 'isic2017.zip'))
    Z.write_config(str(tmp_path), isic2017=str(tmp_path / 'isic2017.zip'))
    monkeypatch.chdir(tmp_path)
    ds = datasets.load_dataset('isic2017', -1, 131, -1, -1, 12345, None)
    ndx, src, net = ds['val_ndx_tgt'], ds['ds_src'], _SpeckleNet()
    run_ = tc.DatasetRun.for_evaluation(ds, ndx, net, torch.device(DEV), 3, torch.float32)
    step = types.SimpleNamespace(align_corners=True)
    got = {}
    for tag, fill in (('filled', True), ('plain', False)):
        sf = evaluation.EvaluatorSurface(2)
        run_.staged_eval(net, step, ndx, evaluation.EvaluatorIoU(2, fill), str(tmp_path / tag), surface=sf)
        got[tag] = sf
    pairs, holes = dict(plain=[], filled=[]), 0
    for i in ndx:
        t = run_.pool.labels(int(i))
        name = src.sample_names[int(i)] + '.png'
        saved = np.asarray(Image.open(tmp_path / 'filled' / name))
        assert np.array_equal(saved, np.asarray(Image.open(tmp_path / 'plain' / name)))          # the plain prediction both times
        maps = dict(plain=_crop(saved, t.shape).astype(np.uint8),
                    filled=_crop(ndimage.binary_fill_holes(saved != 0), t.shape).astype(np.uint8))
        holes += int((maps['plain'] != maps['filled']).sum())
        for tag, p in maps.items():
            pairs[tag].append((t, p))
    print('pixels the hole filling changes:', holes)
    assert holes > 0
    for tag, sf in got.items():
        want = R.dataset([R.reference(t[None], p[None], 2) for t, p in pairs[tag]])
        for have, key in ((sf.hd(), 'hd'), (sf.hd95(), 'hd95'), (sf.assd(), 'assd')):
            _close(have, want[key])
        assert [a.tolist() for a in sf.pairs()] == [want['scored'].tolist(), want['one_sided'].tolist()]
    assert not np.array_equal(got['filled'].assd(), got['plain'].assd())
