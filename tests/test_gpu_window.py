"""
GPU: sliding-window evaluation (csrc/window.hip through ops.window_crop / ops.window_vote, tta.Windows, TTA.predict(windows=...),
EvaluatorIoU.sample_windows, DatasetRun.staged_eval(windows=...), eval_seg --window) against the fp64 restatement of
tests/_window_refs.py, against ops.tta_resize / ops.tta_vote (bit for bit where the definition says so), and end to end on a fabricated
Pascal VOC tree with a small DeepLab v2. Every output is poisoned before the launch and sits between guard bytes that must survive it.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _pascal_tree
import _tta_refs as T
import _window_refs as R

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


def vote(cs, logits=None, labels=None, cm=None, want_pred=True, n=None):
    """ops.window_vote on a case with a poisoned, guarded prediction buffer -> (cm | None, pred | None) on the host"""
    from cutmix_semisup_seg_amd import ops
    _, H, W = R.OUT
    n = R.OUT[0] if n is None else n
    logits = [cu(l) for l in cs['logits']] if logits is None else logits
    g = Guarded((n, H, W), torch.uint8) if want_pred else None
    cm_out, pred = ops.window_vote(logits, cs['flips'], cs['view_sizes'], cs['window'], cs['stride'], cs['c'], (H, W), labels=labels,
                                   align_corners=cs['align'], cm=cm, pred=g.t if g is not None else None)
    torch.cuda.synchronize()
    assert g is None or (g.intact() and pred is g.t)
    return (None if cm_out is None else cm_out.cpu().numpy()), (None if pred is None else pred.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ the crop
CROPS = [(R.CANVAS, False, R.WIN, R.STRIDE), (R.CANVAS, True, R.WIN, R.STRIDE), (R.HALF, True, R.WIN, R.STRIDE),
         (R.LARGE, False, R.WIN, R.WIN), (R.LARGE, True, R.WIN, (4, 6)), (R.SMALL, True, R.WIN, R.STRIDE), ((12, 53), False, R.WIN, R.STRIDE),
         (R.CANVAS, False, (40, 56), (27, 38))]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('view,flip,window,stride', CROPS)
def test_crop_is_resize_plus_slicing_bit_for_bit(dtype, view, flip, window, stride):
    from cutmix_semisup_seg_amd import ops
    from cutmix_semisup_seg_amd.tta import Windows
    x = cu(T.resize_input((2, 3, 37, 53))).to(dtype)
    w = Windows(window, stride)
    (gy, gx), (eh, ew), (ys, xs) = w.grid(view), w.extent(view), w.origins(view)
    g = Guarded((2 * gy * gx, 3, eh, ew), dtype)                          # 0xFF bytes: NaN in fp32 and in bf16
    got = ops.window_crop(x, view, flip, window, stride, out=g.t)
    torch.cuda.synchronize()
    assert got is g.t and g.intact() and not torch.isnan(got).any()       # every element was written
    full = x if (view == R.CANVAS and not flip) else ops.tta_resize(x, view, flip=flip)
    for n in range(2):
        for j, y1 in enumerate(ys):
            for i, x1 in enumerate(xs):
                assert torch.equal(got[(n * gy + j) * gx + i], full[n, :, y1:y1 + eh, x1:x1 + ew])
    assert torch.equal(ops.window_crop(x, view, flip, window, stride), got)


# ------------------------------------------------------------------------------------------------------------------ the vote
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_vote_vs_restatement(name):
    cs = R.case(name)
    assert cs['gap'].min() > R.GAP_BOUND             # a condition on the INPUTS, not a tolerance (tests/test_window_cpu.py)
    labels = cu(cs['labels'])
    cm, pred = vote(cs, labels=labels)
    print(name, 'pixels that differ:', int((pred != cs['pred']).sum()), 'min gap', cs['gap'].min())
    assert np.array_equal(pred, cs['pred'])
    assert np.array_equal(cm, cs['cm'])
    # accumulation into a given matrix, the histogram alone, the prediction alone
    acc = cu(cs['cm'].astype(np.int64))
    cm2, none = vote(cs, labels=labels, cm=acc, want_pred=False)
    assert none is None and np.array_equal(acc.cpu().numpy(), 2 * cs['cm'])
    cm3, pred3 = vote(cs)
    assert cm3 is None and np.array_equal(pred3, cs['pred'])


def test_determinism_and_batch_independence():
    cs = R.case('mixed_c21_k5_a0')
    n = R.OUT[0]
    logits, labels = [cu(l) for l in cs['logits']], cu(cs['labels'])
    a = vote(cs, logits, labels=labels)
    b = vote(cs, logits, labels=labels)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    total = np.zeros_like(a[0])
    for i in range(n):
        own = [l[i * (l.shape[0] // n):(i + 1) * (l.shape[0] // n)].contiguous() for l in logits]
        cm, pred = vote(cs, own, labels=labels[i:i + 1].contiguous(), n=1)
        assert np.array_equal(pred[0], a[1][i])
        total += cm
    assert np.array_equal(total, a[0])


@pytest.mark.parametrize('k,c', [(1, 21), (2, 19), (5, 19), (16, 64)])
def test_a_window_that_holds_every_view_is_tta_vote_bit_for_bit(k, c):
    from cutmix_semisup_seg_amd import ops
    n, H, W = T.OUT
    lg, flips = T.make_views(k, c, n, seed=k + c)
    logits, labels = [cu(l) for l in lg], cu(T.make_labels((n, H, W), c, 5))
    want_cm, want_pred = ops.tta_vote(logits, flips, c, (H, W), labels=labels, align_corners=False, want_pred=True)
    g = Guarded((n, H, W), torch.uint8)
    cm, pred = ops.window_vote(logits, flips, [tuple(l.shape[2:]) for l in lg], (64, 96), (43, 64), c, (H, W), labels=labels,
                               align_corners=False, pred=g.t)
    torch.cuda.synchronize()
    assert g.intact() and torch.equal(pred, want_pred) and torch.equal(cm, want_cm)
    # the views larger than their logits (what a network makes of them): still one window each, still the vote
    cm, pred = ops.window_vote(logits, flips, [(64, 96)] * k, (64, 96), (16, 24), c, (H, W), labels=labels, align_corners=False,
                               want_pred=True)
    assert torch.equal(pred, want_pred) and torch.equal(cm, want_cm)


def test_sample_windows_with_fill_holes():
    from cutmix_semisup_seg_amd import evaluation, ops
    from cutmix_semisup_seg_amd.tta import Windows
    cs = R.case('dense_c2_k2_a1')
    n, H, W = R.OUT
    logits = [cu(l) for l in cs['logits']]
    truth = cu(np.where(cs['labels'] == 255, 255, cs['labels'] % 2).astype(np.uint8))
    w = Windows(cs['window'], cs['stride'])
    ev = evaluation.EvaluatorIoU(2, fill_holes=True)
    ev.sample_windows(logits, cs['flips'], cs['view_sizes'], w, truth[:, None], (H, W), ignore_value=255, align_corners=cs['align'])
    filled, want_cm = ops.fill_holes(cu(cs['pred']), truth=truth, ignore_index=255)
    assert np.array_equal(ev.cm, want_cm.cpu().numpy().astype(np.float64))
    plain = evaluation.EvaluatorIoU(2)
    plain.sample_windows(logits, cs['flips'], cs['view_sizes'], w, truth, (H, W), ignore_value=255, align_corners=cs['align'])
    assert np.array_equal(plain.cm, T.confusion(truth.cpu().numpy(), cs['pred'], 2).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ refusals
def _desc(cs, logits, pred, labels=None, cm=None):
    from cutmix_semisup_seg_amd import _lib
    n, H, W = R.OUT
    d = _lib.WindowDesc()
    for i, (t, v) in enumerate(zip(logits, cs['layout'])):
        d.logits[i] = t.data_ptr()
        for name in ('hl', 'wl', 'Hv', 'Wv', 'gy', 'gx', 'eh', 'ew'):
            getattr(d, name)[i] = v[name]
        d.sh[i], d.sw[i], d.flip[i] = cs['stride'][0], cs['stride'][1], int(v['flip'])
    d.wh, d.ww = cs['window']
    d.n, d.c, d.H, d.W, d.k, d.align_corners = n, cs['c'], H, W, len(logits), int(cs['align'])
    d.labels = None if labels is None else labels.data_ptr()
    d.label_dtype, d.ignore_index = _lib.LABEL_U8, 255
    d.cm = None if cm is None else cm.data_ptr()
    d.pred_out = pred.data_ptr()
    return d


def test_refusals_are_einval_and_launch_nothing():
    from cutmix_semisup_seg_amd import _lib
    cs = R.case('half_c21_k2_a1')
    n, H, W = R.OUT
    logits = [cu(l) for l in cs['logits']]
    g = Guarded((n, H, W), torch.uint8, poison=0x5A)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(change):
        d = _desc(cs, logits, g.t)
        change(d)
        return _lib.fn['cms_window_vote'](ctypes.byref(d), stream)

    def seti(field, i, value):
        return lambda d: getattr(d, field).__setitem__(i, value)
    changes = [lambda d: setattr(d, 'n', 0), lambda d: setattr(d, 'c', 65), lambda d: setattr(d, 'k', 17), lambda d: setattr(d, 'H', 0),
               lambda d: setattr(d, 'wh', 0), lambda d: setattr(d, 'ww', 23), lambda d: setattr(d, 'pred_out', None),
               lambda d: setattr(d, 'cm', g.t.data_ptr()), lambda d: d.logits.__setitem__(1, None),
               seti('sh', 0, 0), seti('sw', 1, 25), seti('sh', 1, 17), seti('sh', 0, 3), seti('sw', 0, 5), seti('eh', 0, 15),
               seti('ew', 1, 27), seti('gy', 0, 4), seti('gx', 1, 1), seti('Hv', 0, 49), seti('Wv', 1, 0), seti('hl', 0, 17),
               seti('wl', 1, 25), seti('hl', 1, 0)]
    for ch in changes:
        assert call(ch) == -1 and _lib.fn['cms_last_error']()
    assert _lib.fn['cms_window_vote'](None, stream) == -1
    x = cu(T.resize_input((1, 3, 9, 11)))
    out = Guarded((4, 3, 6, 8), torch.float32, poison=0x5A)
    crop = _lib.fn['cms_window_crop']
    for args in ((x.data_ptr(), None, 1, 3, 9, 11, 9, 11, 0, 6, 8, 4, 5, 0), (None, out.t.data_ptr(), 1, 3, 9, 11, 9, 11, 0, 6, 8, 4, 5, 0),
                 (x.data_ptr(), out.t.data_ptr(), 1, 3, 9, 11, 9, 11, 0, 6, 8, 7, 5, 0),          # a stride above its window
                 (x.data_ptr(), out.t.data_ptr(), 1, 3, 9, 11, 9, 11, 0, 6, 8, 1, 5, 0),          # ... below ceil(window / 4)
                 (x.data_ptr(), out.t.data_ptr(), 1, 3, 9, 11, 9, 11, 0, 0, 8, 4, 5, 0),
                 (x.data_ptr(), out.t.data_ptr(), 1, 3, 9, 11, 0, 11, 0, 6, 8, 4, 5, 0),
                 (x.data_ptr(), out.t.data_ptr(), 0, 3, 9, 11, 9, 11, 0, 6, 8, 4, 5, 0),
                 (x.data_ptr(), out.t.data_ptr(), 1, 3, 9, 11, 9, 11, 0, 6, 8, 4, 5, 7),          # an unknown dtype
                 (x.data_ptr(), out.t.data_ptr(), 2 ** 20, 3, 9, 11, 2 ** 15, 2 ** 15, 0, 6, 8, 4, 5, 0)):
        assert crop(*args, stream) == -1
    torch.cuda.synchronize()
    assert g.intact() and bool((g.t == 0x5A).all()) and out.intact() and bool((out.buf[GUARD:-GUARD] == 0x5A).all())
    # the untouched descriptor is taken
    assert call(lambda d: None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(g.t.cpu().numpy(), cs['pred'])


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZE = (80, 104)
VAL = ['img_a', 'img_b', 'img_c', 'img_d']
SIZES = dict({name: SIZE for name in VAL}, img_e=SIZE)
HALF_WINDOW = (40, 52)                      # default stride (27, 35): 3 x 3 windows on the (80, 104) canvas


@pytest.fixture(scope='module')
def pascal(tmp_path_factory):
    """-> (working directory with a tree of images of ONE size and its configuration, model.pth of a small DeepLab v2)"""
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    cwd = tmp_path_factory.mktemp('window_pascal')
    root = _pascal_tree.write_tree(str(cwd / 'VOC2012'), SIZES, ['img_e'], VAL)
    _pascal_tree.write_config(str(cwd), root)
    from oracle import deeplab2 as odl
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(21, [1, 1, 1, 1]))      # weights under which the classes are not tied
    model_path = str(cwd / 'model.pth')
    checkpoint.save_model(net, model_path)
    return cwd, model_path


def _evaluate(model_path, capsys, save, **kw):
    import eval_seg
    iou = eval_seg.evaluate(model_path, 'pascal', batch_size=3, compute_dtype='fp32', save_preds=str(save), **kw)
    return iou, [l for l in capsys.readouterr().out.splitlines() if l.startswith('VAL mIoU=') or l.startswith('-- ')]


def _files(d):
    from PIL import Image
    assert sorted(os.listdir(d)) == sorted(n + '.png' for n in VAL)
    return {n: np.asarray(Image.open(os.path.join(str(d), n + '.png'))) for n in VAL}


def test_eval_seg_window_that_holds_the_canvas_changes_nothing(pascal, monkeypatch, tmp_path, capsys):
    cwd, model_path = pascal
    monkeypatch.chdir(cwd)
    for name, extra in (('one', {}), ('six', dict(scales='0.75,1,1.25', flip=True))):
        want, want_lines = _evaluate(model_path, capsys, tmp_path / (name + '_plain'), **extra)
        got, lines = _evaluate(model_path, capsys, tmp_path / (name + '_window'), window='160,208', **extra)
        assert np.array_equal(got, want) and want.sum() > 0
        a, b = _files(tmp_path / (name + '_plain')), _files(tmp_path / (name + '_window'))
        assert all(np.array_equal(a[n], b[n]) for n in VAL)
        views = 1 if name == 'one' else 6
        assert lines[:2] == want_lines[:2] and lines[2:] == [
            '-- sliding window 160x208 stride 107x139: {} windows over 4 images'.format(4 * views)]
        assert len(want_lines) == 2


def _torch_stitch(logits, flips, sizes, windows, canvas, align):
    """the definition with torch operations: upsample every window, softmax, add into a view canvas beside a count map, divide, read
    the view at every canvas pixel, sum the views, argmax"""
    import torch.nn.functional as F
    H, W = canvas
    score = 0.0
    for l, flip, view in zip(logits, flips, sizes):
        (gy, gx), (eh, ew), (ys, xs) = windows.grid(view), windows.extent(view), windows.origins(view)
        n = l.shape[0] // (gy * gx)
        if gy * gx == 1:                    # one window holds the view: read as the vote over whole views reads it
            up = F.interpolate(l.float(), size=canvas, mode='bilinear', align_corners=align)
            score = score + (up.flip(-1) if flip else up).softmax(1)
            continue
        p = F.interpolate(l.float(), size=(eh, ew), mode='bilinear', align_corners=align).softmax(1).view(n, gy, gx, -1, eh, ew)
        acc = torch.zeros((n, l.shape[1]) + tuple(view), device=l.device)
        cnt = torch.zeros(tuple(view), device=l.device)
        for j, y1 in enumerate(ys):
            for i, x1 in enumerate(xs):
                acc[:, :, y1:y1 + eh, x1:x1 + ew] += p[:, j, i]
                cnt[y1:y1 + eh, x1:x1 + ew] += 1
        ry, rx = cu(R.view_coord(H, view[0])), cu(R.view_coord(W, view[1]))
        if flip:
            rx = view[1] - 1 - rx
        score = score + (acc / cnt)[:, :, ry[:, None], rx[None, :]]
    return score.argmax(1)


@pytest.mark.parametrize('views', ['one', 'six'])
def test_eval_seg_half_window_end_to_end(pascal, monkeypatch, tmp_path, capsys, views):
    from cutmix_semisup_seg_amd import checkpoint, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets, seg_data
    from cutmix_semisup_seg_amd.tta import TTA, Windows
    cwd, model_path = pascal
    monkeypatch.chdir(cwd)
    extra = {} if views == 'one' else dict(scales='0.75,1,1.25', flip=True)
    tta = TTA((1.0,), False) if views == 'one' else TTA((0.75, 1, 1.25), True)
    iou, lines = _evaluate(model_path, capsys, tmp_path / 'half', window='40,52', window_batch=4, **extra)
    windows = Windows(HALF_WINDOW)
    assert windows.stride == (27, 35) and windows.grid(SIZE) == (3, 3)
    per_image = tta.window_count(SIZE, (1, 1), windows)
    assert per_image == (9 if views == 'one' else 2 * (windows.count((60, 78)) + 9 + windows.count((100, 130))))
    assert lines[2:] == ['-- sliding window 40x52 stride 27x35: {} windows over 4 images'.format(4 * per_image)]
    saved = _files(tmp_path / 'half')
    if views == 'one':                     # the command line says and saves the same
        from click.testing import CliRunner
        import eval_seg
        res = CliRunner().invoke(eval_seg.experiment, [model_path, '--dataset', 'pascal', '--batch_size', '3', '--compute_dtype', 'fp32',
                                                       '--window', '40,52', '--window_stride', '27,35', '--window_batch', '4',
                                                       '--save_preds', str(tmp_path / 'cli')], catch_exceptions=False)
        assert res.exit_code == 0, res.output
        assert [l for l in res.output.splitlines() if l.startswith('VAL mIoU=') or l.startswith('-- ')] == lines
        cli = _files(tmp_path / 'cli')
        assert all(np.array_equal(cli[n], saved[n]) for n in VAL)

    ds = datasets.load_dataset('pascal', -1, 131, -1, -1, 12345, None)
    net = checkpoint.load_model(model_path).to(DEV)
    net.compute_dtype = torch.float32
    net.eval()
    run = tc.DatasetRun.for_evaluation(ds, ds['val_ndx_tgt'], net, torch.device(DEV), 3, torch.float32)
    flips = [f for _, f in tta.views()]
    pixels = outside = forwarded = 0
    cm = np.zeros((21, 21), dtype=np.int64)
    with torch.no_grad():
        for batch in seg_data.eval_batches(run.val_ndx, run.batch_size):
            ev = run.augment.stage_eval(run.pool, batch, net.BLOCK_SIZE)
            assert ev['canvas'] == SIZE
            logits, sizes = tta.forward_windows(net, ev['image'], windows, net.BLOCK_SIZE, 4)
            forwarded += sum(int(l.shape[0]) for l in logits)
            want = _torch_stitch(logits, flips, sizes, windows, SIZE, net.upsample_align_corners).cpu().numpy()
            _, ref, gap = R.stitch([l.cpu().numpy() for l in logits], flips, sizes, windows.window, windows.stride, SIZE,
                                   net.upsample_align_corners)
            sure = gap > R.GAP_BOUND
            pixels += sure.size
            outside += int((~sure).sum())
            labels = ev['labels'][:, 0].cpu().numpy()
            for k, i in enumerate(batch):
                got = saved[ds['ds_src'].sample_names[i]]
                assert np.array_equal(got[sure[k]], want[k][sure[k]]) and np.array_equal(got[sure[k]], ref[k][sure[k]])
                cm += T.confusion(labels[k], got.astype(np.uint8), 21)
    assert forwarded == 4 * per_image
    print(views, 'pixels the restatement does not decide by more than the gap bound:', outside, 'of', pixels)
    assert outside <= 0.01 * pixels                       # a condition on the inputs: the rule above covers at least 99 % of the pixels
    # the printed IoU is the IoU of the saved files
    inter, total = np.diag(cm).astype(np.float64), (cm.sum(0) + cm.sum(1) - np.diag(cm)).astype(np.float64)
    assert np.allclose(iou[total > 0], (inter / np.maximum(total, 1))[total > 0], rtol=0, atol=1e-12)
    print(views, 'classes predicted:', np.count_nonzero(cm.sum(axis=0)))
    if views == 'one':
        assert np.count_nonzero(cm.sum(axis=0)) > 1       # the network predicts more than one class (six views agree on one)
