"""
GPU: the bandwidth-bound kernels around the convolutions -- csrc/nhwc.hip, aspp.hip, upsample.hip, eval.hip, optim.hip, the
max-pool of stem.hip and the deferred factor of the one-launch losses -- against the plain fp64 references of
tests/_stream_refs.py (pinned against torch on the CPU by tests/test_stream_refs_cpu.py), at sizes that reach what moves the bytes
at real sizes: the unrolled main loops, the tails behind them, and the second trip of every grid-stride loop.

Tolerances are derived, not tuned: an output that is a sum of products accumulated in fp32 must satisfy, on EVERY element,

    |got - ref| <= (d + 2) * u32 * A  [+ u_bf * |ref| when stored as bf16]         (_stream_refs.bound; d stated at each use)

and data movement (copies, concat, spread, pooling, the pool-backward scatter of integer gradients, confusion counts) is exact.
Each check prints `RATIO <what> <largest |got - ref| / bound>` before it asserts ("streaming-kernel tests").
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _stream_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ['fp32', 'bf16']
W32 = np.float32            # bilinear weights of an fp32 implementation of the definition (see _stream_refs)


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


def _randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _ints(shape, dtype, seed, lim=8):
    """integers |v| <= lim: exact in bf16, and every partial sum of the cases below stays < 2^24"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).to(dtype)


def _np(t):
    """device / host tensor of either dtype -> fp64 numpy (bf16 and fp32 are exact in fp64)"""
    return t.detach().float().cpu().numpy().astype(np.float64)


def _rne(a, dtype):
    """fp64 numpy array -> the value an fp32 accumulator holding it exactly would store as `dtype` (round to nearest even)"""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype)


def _bf(dtype):
    return dtype == torch.bfloat16


def _dn(dtype):
    return 'bf16' if dtype == torch.bfloat16 else 'fp32'


# ====================================================================================================== nhwc: rows_reduce
_ROWS = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 96: (8, 12), 97: (1, 97), 127: (1, 127), 128: (8, 16), 129: (3, 43),
         1089: (33, 33), 16641: (129, 129)}


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('rows', sorted(_ROWS))
def test_global_avg_pool_main_loop_and_tails(ops, rows, dtype):
    """hole 1: rows_reduce_kernel's four-way unrolled loop (p + 96 < rows), the 32-row tail loop behind it and slots that see no row
    at all, for channel counts with full and partial 64-channel tiles. Forward = mean (d = ceil(rows / 32) + 32: a slot's serial
    chain, then the serial sum over the 32 slots; the scale factor is one of the "+ 2"); backward = the row-broadcast copy."""
    H, W = _ROWS[rows]
    for N in (1, 3):
        for Cc in (8, 64, 72, 304):
            x = _randn((N, H, W, Cc), dtype, rows * 7 + Cc + N)
            g = _randn((N, 1, 1, Cc), dtype, rows * 11 + Cc + N)
            xd = x.to(DEV).requires_grad_(True)
            out = ops.global_avg_pool(xd)
            out.backward(g.to(DEV))
            ref, A = R.mean_over_pixels(_np(x))
            R.assert_within(_np(out), ref, R.bound(A, R.rows_reduce_depth(rows), ref, _bf(dtype)),
                            'rows_reduce {} mean rows={} C={} N={}'.format(_dn(dtype), rows, Cc, N))
            # backward: (g * (1 / rows)) rounded to the dtype, copied to every pixel: one product (d = 0)
            gref = np.broadcast_to(_np(g) / rows, (N, H, W, Cc))
            R.assert_within(_np(xd.grad), gref, R.bound(np.abs(gref), 0, gref, _bf(dtype)), 'row_broadcast {} avg_pool bwd rows={}'.format(_dn(dtype), rows))
            assert torch.equal(xd.grad, xd.grad[:, :1, :1, :].expand(N, H, W, Cc))            # and the same bits on every pixel


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('rows', sorted(_ROWS))
def test_rows_reduce_exact_integer_sums(ops, rows, dtype):
    """hole 1, order-free: integer inputs |v| <= 8 and scale = 1 -- every partial sum is exact in fp32, so the result is the integer
    sum bit for bit whatever the summation order; a dropped, doubled or misrouted row shows. Rows live in wider rows (pitch != C)
    at a non-zero channel offset, as in the broadcast branch's gradient."""
    from cutmix_semisup_seg_amd._lib import fn, check
    H, W = _ROWS[rows]
    for N in (1, 3):
        for Cc in (8, 64, 72, 304):
            pitch, off = Cc + 24, 16
            buf = _ints((N, H, W, pitch), dtype, rows * 13 + Cc + N).to(DEV)
            acc = torch.full((N, Cc), -77.0, dtype=torch.float32, device=DEV)
            check(fn['cms_rows_reduce'](buf.data_ptr() + off * buf.element_size(), pitch, N, rows, Cc, ops._dtype_code(buf),
                                        acc.data_ptr(), 1.0, ops._stream()), 'cms_rows_reduce')
            want = _np(buf)[..., off:off + Cc].sum(axis=(1, 2))
            assert np.array_equal(_np(acc), want), 'rows={} C={} N={}'.format(rows, Cc, N)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('hw', [(33, 33), (129, 129)], ids=['33x33', '129x129'])
@pytest.mark.parametrize('exact', [False, True], ids=['randn', 'integers'])
def test_concat_broadcast_gradient_pitch_and_offset(ops, hw, dtype, exact):
    """hole 1: the pooled branch's gradient = rows_reduce over a channel slice of the concat gradient (pitch = all channels, pointer
    offset != 0: the broadcast input is not the first) at 33 x 33 and 129 x 129 rows. Forward and the other gradients are copies."""
    H, W = hw
    N, cs = 2, (48, 72, 8)
    mk = _ints if exact else _randn
    xs = [mk((N, H, W, cs[0]), dtype, 1), mk((N, 1, 1, cs[1]), dtype, 2), mk((N, H, W, cs[2]), dtype, 3)]
    dy = mk((N, H, W, sum(cs)), dtype, 4)
    dev_in = [x.to(DEV).requires_grad_(True) for x in xs]
    out = ops.concat_channels(dev_in)
    out.backward(dy.to(DEV))
    assert np.array_equal(_np(out), R.concat_broadcast([_np(x) for x in xs]))
    refs = R.concat_broadcast_adjoint(_np(dy), [tuple(x.shape) for x in xs])
    for i, (xd, (ref, A)) in enumerate(zip(dev_in, refs)):
        if i != 1:
            assert np.array_equal(_np(xd.grad), ref)
        elif exact:
            assert torch.equal(xd.grad.cpu(), _rne(ref, dtype)), 'integer sums (rounded once to the dtype)'
        else:
            R.assert_within(_np(xd.grad), ref, R.bound(A, R.rows_reduce_depth(H * W), ref, _bf(dtype)),
                            'rows_reduce {} concat-grad {}x{}'.format(_dn(dtype), H, W))


# ====================================================================================================== nhwc: copies
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_channel_copy_wraps_the_grid_and_stays_in_its_slice(ops, dtype):
    """hole 2: 2 x 129 x 129 rows of 304 channels into rows of 352 = 1.26 M (bf16) / 2.5 M (fp32) 16-byte chunks > 256 x 4096
    threads: the second trip of channel_copy_kernel's grid-stride loop and its i / chunks split. The neighbouring slice holds a
    sentinel and must stay untouched; then the same slice back out (pitch on the source side), and a row-broadcast copy."""
    N, H, W, cl, cx = 2, 129, 129, 48, 304
    rows = N * H * W
    src = _randn((N, H, W, cx), dtype, 5).to(DEV)
    dst = torch.full((N, H, W, cl + cx), 7.0, dtype=dtype, device=DEV)
    ops._channel_copy(src, 0, cx, dst, cl, cl + cx, rows, cx)
    assert torch.equal(dst[..., cl:], src)
    assert bool((dst[..., :cl] == 7.0).all())
    back = torch.full((N, H, W, cx), -1.0, dtype=dtype, device=DEV)
    ops._channel_copy(dst, cl, cl + cx, back, 0, cx, rows, cx)
    assert torch.equal(back, src)
    row = _randn((N, 1, 1, cx), dtype, 6).to(DEV)
    dst.fill_(7.0)
    ops._channel_copy(row, 0, cx, dst, cl, cl + cx, rows, cx, row_div=H * W)
    assert torch.equal(dst[..., cl:], row.expand(N, H, W, cx))
    assert bool((dst[..., :cl] == 7.0).all())


# ====================================================================================================== nhwc: add_n
_FAN_SHAPES = [(1, 1, 1, 8), (2, 5, 7, 24), (1, 33, 33, 304)]
_FAN_BIG = (2, 129, 129, 256)                 # numel / 8 = 1 064 992 > 256 x 4096: add_n_kernel's loop wraps


def _fanout_grad(ops, x, gs):
    xd = x.to(DEV).requires_grad_(True)
    al = ops.fanout(xd, len(gs))
    live = [(a, g.to(DEV)) for a, g in zip(al, gs) if g is not None]
    torch.autograd.backward([a for a, _ in live], [g for _, g in live])
    return xd.grad


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 6, 7])
def test_fanout_sums_k_gradients(ops, k, dtype):
    """hole 3: add_n_kernel with every source count 2..6 (the unused pointer slots are padded with source 0 and must not be added),
    k = 1 (passed through) and k = 7 (the torch fallback); for k <= 5 also with one alias nobody consumed, whose gradient autograd
    materialises as zeros (k + 1 sources). fp32 accumulation of n sources: d = n - 1. Integer inputs: exact."""
    shapes = _FAN_SHAPES + ([_FAN_BIG] if k in (2, 6) else [])
    for shape in shapes:
        x = _randn(shape, dtype, 1)
        for exact in (True, False):
            if k == 7 and not exact and _bf(dtype):
                continue                   # (the fallback adds pairwise in bf16: only its integer sums are comparable)
            gs = [(_ints if exact else _randn)(shape, dtype, 10 + j) for j in range(k)]
            ref, A = R.sum_k([_np(g) for g in gs])
            for unused in ((False, True) if k <= 5 and shape != _FAN_BIG else (False,)):
                pos = k // 2
                got = _fanout_grad(ops, x, gs[:pos] + [None] + gs[pos:] if unused else gs)
                if exact:
                    assert np.array_equal(_np(got), ref), 'k={} shape={}'.format(k, shape)
                else:
                    R.assert_within(_np(got), ref, R.bound(A, k - 1 + int(unused), ref, _bf(dtype)),
                                    'add_n {} k={} numel={}'.format(_dn(dtype), k + int(unused), x.numel()))


# ====================================================================================================== nhwc: bilinear
_UP_CASES = [(g, 2, 8, 16) for g in R.BILINEAR_GEOS] + [(((33, 33), (129, 129)), 2, 48, 304),      # forward: 1.26 M work items
                                                         (R.NHWC_WRAP_GEO, 2, 8, 256)]               # adjoint: 1.06 M work items
_up_id = lambda c: '{}x{}to{}x{}_C{}'.format(c[0][0][0], c[0][0][1], c[0][1][0], c[0][1][1], c[3])


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('align', [False, True], ids=['half_pixel', 'align_corners'])
@pytest.mark.parametrize('case', _UP_CASES, ids=_up_id)
def test_upsample_concat_forward_and_adjoint(ops, case, align, dtype):
    """holes 2 and 4: upsample_nhwc_fwd_kernel (d = 3: four products) into its channel slice next to the copied `low` slice, and the
    gather-form adjoint (upsample_nhwc_bwd_kernel / adjoint_range; d = the number of output pixels that touch the source pixel) at
    size-1 sources and outputs, non-integer ratios both ways, ratios above 4, and two sizes that wrap the grid. The reference uses
    the fp32 bilinear weights of the definition. In fp32 also <U x, y> = <x, U^T y> in fp64 from the device outputs, to within the
    two bounds summed against the other factor."""
    ((h, w), (H, W)), N, cl, cx = case
    low = _randn((N, H, W, cl), dtype, 1)
    x = _randn((N, h, w, cx), dtype, 2)
    dy = _randn((N, H, W, cl + cx), dtype, 3)
    ld, xd = low.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    out = ops.upsample_concat(ld, xd, align_corners=align)
    out.backward(dy.to(DEV))
    assert torch.equal(out[..., :cl].cpu(), low) and torch.equal(ld.grad.cpu(), dy[..., :cl])          # copies
    ref, A = R.upsample_bilinear(_np(x), (H, W), align, 'nhwc', W32)
    bf = R.bound(A, 3, ref, _bf(dtype))
    R.assert_within(_np(out[..., cl:]), ref, bf, 'upsample_nhwc_fwd {} {} align={}'.format(_dn(dtype), _up_id(case), int(align)))
    gy = _np(dy)[..., cl:]
    adj, Aa, d = R.upsample_bilinear_adjoint(gy, (h, w), align, 'nhwc', W32)
    ba = R.bound(Aa, d, adj, _bf(dtype))
    R.assert_within(_np(xd.grad), adj, ba, 'upsample_nhwc_adjoint {} {} align={}'.format(_dn(dtype), _up_id(case), int(align)))
    if dtype == torch.float32:
        lhs, rhs = R.dot64(_np(out[..., cl:]), gy), R.dot64(_np(x), _np(xd.grad))
        assert abs(lhs - rhs) <= float((bf * np.abs(gy)).sum() + (ba * np.abs(_np(x))).sum()), (lhs, rhs)


# ====================================================================================================== aspp
def _taps18(ops):
    return ops.conv_taps(3, 3, 6, 6) + ops.conv_taps(3, 3, 12, 12)


@pytest.mark.parametrize('Cc', R.ASPP_CLASSES)
@pytest.mark.parametrize('nhw', R.ASPP_MAPS, ids=lambda m: 'x'.join(map(str, m)))
def test_aspp_gather_and_spread(ops, nhw, Cc):
    """hole 5 (and 2): the shift-gather (fp32 serial sum of bias and T shifted planes: d = T) with and without bias, and the spread in
    fp32 AND bf16 (the instantiation the timed engine uses) -- exact, zeros in the columns >= T * C included -- for class counts
    below 8 (one 8-column chunk spans several taps), 19 and 21; 18 taps of dilation 6 / 12 and a single off-centre tap; ZC = T * C
    rounded up to 128 and to 8; maps from one pixel, over one smaller than the dilation (every off-centre tap outside), to
    4 x 65 x 129 (C = 19 / 21: ZC = 384, 1.6 M chunks -- the spread's grid-stride loop and 32-bit index split wrap; C = 2 / 5 get an
    N = 8 run for the same, 1.07 M chunks at ZC = 128; with C = 21 and N = 7 the gather's loop wraps too).
    <gather(Z), dL> = <Z, spread(dL)> in fp64 from the device outputs, to within the gather's bound summed against |dL|."""
    N, H, W = nhw
    runs = [(N, _taps18(ops)), (N, [(-3, 2)])]
    if Cc == 21 and H * W > 8000:
        runs.append((7, _taps18(ops)))                    # 7 * 21 * 65 * 129 = 1 232 595 logits > 256 x 4096
    if Cc < 8 and H * W > 8000:
        runs.append((8, _taps18(ops)))                    # 8 * 65 * 129 * 128 / 8 = 1 073 280 chunks: the C < 8 walk on a second trip
    for n, taps in runs:
        T = len(taps)
        for zc in sorted({(T * Cc + 127) // 128 * 128, (T * Cc + 7) // 8 * 8}):
            z = _randn((n, zc, H, W), torch.float32, Cc * 10 + T)
            bias = _randn((Cc,), torch.float32, 5)
            dl = _randn((n, Cc, H, W), torch.float32, 6)
            zd, dld = z.to(DEV), dl.to(DEV)
            tag = 'aspp_gather fp32 C={} T={} zc={} map={}x{}x{}'.format(Cc, T, zc, n, H, W)
            got0 = None
            for b in (bias, None):
                got = ops.aspp_gather_fwd(zd, None if b is None else b.to(DEV), taps, Cc)
                ref, A = R.aspp_gather(_np(z), None if b is None else _np(b), taps, Cc)
                bnd = R.bound(A, T)
                R.assert_within(_np(got), ref, bnd, tag + (' bias' if b is not None else ' bias=None'))
                got0 = got
            want = R.aspp_spread(dl.numpy(), taps, zc)
            for dt in DTYPES:
                D = ops.aspp_spread_bwd(dld, taps, zc, dt)
                assert torch.equal(D.cpu(), torch.from_numpy(want).to(dt)), tag + ' spread ' + str(dt)
                assert not bool(D[..., T * Cc:].any())
            D32 = ops.aspp_spread_bwd(dld, taps, zc, torch.float32)
            lhs, rhs = R.dot64(_np(got0), _np(dl)), R.dot64(_np(z), _np(D32).transpose(0, 3, 1, 2))
            assert abs(lhs - rhs) <= float((bnd * np.abs(_np(dl))).sum()), (tag, lhs, rhs)


# ====================================================================================================== stem max-pool
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('ceil_mode', [False, True], ids=['floor', 'ceil'])
@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_forward_index_and_backward(ops, shape, ceil_mode, dtype):
    """hole 6 (and 2): 3 x 3 / 2 max-pool in both ceil modes and both dtypes, odd and even sizes from 1 x 1 to 2 x 257 x 513 x 128
    (forward and backward grids wrap). The inputs are quarter-integers: full of exact ties and exact zeros. Forward: exact; the
    index points inside its window at an element equal to the maximum. Backward: the reference routes dp by the kernel's OWN index
    map and gates by s > 0, so it does not depend on how ties were broken; dp holds small integers, so sums of up to four
    window gradients are exact in either dtype."""
    s = R.pool_input(shape, seed=shape[1] * 31 + shape[2])
    sd = torch.from_numpy(s).to(dtype).to(DEV)
    p, idx = ops.maxpool3x3s2_forward(sd, ceil_mode=ceil_mode)
    want = R.maxpool3x3s2(s, ceil_mode)
    assert tuple(p.shape) == want.shape
    assert np.array_equal(p.float().cpu().numpy(), want)
    idx_h = idx.cpu().numpy().astype(np.int64)
    assert idx_h.max() <= 8
    val, inside = R.maxpool_window_value(s, idx_h, ceil_mode)
    assert inside.all() and np.array_equal(val, want)
    dp = np.random.RandomState(7).randint(-8, 9, size=want.shape).astype(np.float32)
    ds = ops.maxpool3x3s2_relu_backward(torch.from_numpy(dp).to(dtype).to(DEV), idx, sd, ceil_mode=ceil_mode)
    ref = R.maxpool3x3s2_relu_backward(dp, idx_h, s)
    assert np.array_equal(_np(ds), ref)
    assert ref.any() or shape[1] * shape[2] <= 6


# ====================================================================================================== evaluation
def _eval_labels(case, ldt, ignore, seed):
    n, c, h, w, H, W = case[:6]
    rng = np.random.RandomState(seed)
    y = rng.randint(0, c, size=(n, H, W)).astype(np.int64)
    r = rng.rand(n, H, W)
    y[r < 0.05] = 255                                   # the usual ignore value (a plain out-of-range label when ignore is not 255)
    if c < 254:
        m = (r >= 0.05) & (r < 0.08)
        y[m] = rng.randint(c, 255, size=int(m.sum()))   # labels >= C that are not the ignore value
    if ignore is not None and ignore < c:
        y[(r >= 0.08) & (r < 0.12)] = ignore
    if ldt == torch.int64:
        y[(r >= 0.12) & (r < 0.14)] = -1
        y[(r >= 0.14) & (r < 0.15)] = -(2 ** 40)
        y[(r >= 0.15) & (r < 0.17)] = 2 ** 31 + 3       # would alias class 3 if truncated to 32 bits
        y[(r >= 0.17) & (r < 0.18)] = 2 ** 32 + 1
        return torch.from_numpy(y)
    return torch.from_numpy(y.astype(np.uint8))


@pytest.mark.parametrize('case', R.EVAL_CASES, ids=lambda c: 'x'.join(map(str, c[:7])))
def test_argmax_confusion_prediction_and_counts(ops, case):
    """hole 7 (and 2): the fused upsample + argmax + confusion matrix for uint8 and int64 labels (ignore value, values in
    [C, 254], negative and > 2^31 int64 values), ignore_index 255 / None / a real class, both align_corners, the identity path,
    C in {1, 2, 21, 64}, accumulation into a given matrix, and P = 525 825 > 1024 x 256. Counts: integer-exact against bincount of
    the kernel's own prediction. Prediction: against the fp64 upsample (fp32 weights of the definition) -- with eps = 4 u32 max|logit|
    every pixel whose top-1 margin exceeds 2 eps must match exactly, and elsewhere the chosen class lies within 2 eps of the
    maximum (tests/test_stream_refs_cpu.py asserts that such pixels are <= 1e-4 of all for these inputs)."""
    n, c, h, w, H, W, align, _ = case
    lo = R.eval_logits(case)
    lod = torch.from_numpy(lo).to(DEV)
    up, _ = R.upsample_bilinear(lo, (H, W), align, 'nchw', W32)
    eps = 4 * R.U32 * float(np.abs(lo).max())
    top, margin = R.argmax_margin(up)
    pred = first = None
    for ldt in (torch.uint8, torch.int64):
        for ignore in (255, None, 0):
            y = _eval_labels(case, ldt, ignore, 3)
            cm, pred = ops.argmax_confusion(lod, y.to(DEV), c, (H, W), ignore, align, want_pred=True)
            ph = pred.cpu().numpy().astype(np.int64)
            assert first is None or np.array_equal(ph, first), 'the prediction does not depend on the labels'
            first = ph
            assert np.array_equal(cm.cpu().numpy(), R.confusion(y.numpy(), ph, c, ignore)), (ldt, ignore)
            # accumulation into the given matrix, second call with other labels
            y2 = _eval_labels(case, ldt, ignore, 4)
            cm2, _ = ops.argmax_confusion(lod, y2.to(DEV), c, (H, W), ignore, align, cm=cm)
            assert cm2 is cm
            assert np.array_equal(cm.cpu().numpy(), R.confusion(y.numpy(), ph, c, ignore) + R.confusion(y2.numpy(), ph, c, ignore))
    decided = margin > 2 * eps
    assert np.array_equal(ph[decided], top[decided])
    chosen = np.take_along_axis(up, ph[:, None], axis=1)[:, 0]
    assert (chosen >= up.max(axis=1) - 2 * eps).all()
    print('RATIO argmax undecided share {:.6f}'.format(float((~decided).mean())))
    # labels = None: predictions only
    _, p2 = ops.argmax_confusion(lod, None, c, (H, W), 255, align, want_pred=True)
    assert torch.equal(p2, pred)


def test_argmax_ties_and_nan_on_the_identity_path(ops):
    """hole 7: torch.argmax's rules -- the lowest index wins an exact tie, NaN counts as maximal, the first NaN wins"""
    Cc = 5
    lo = _randn((1, Cc, 4, 4), torch.float32, 1)
    lo[0, :, 0, 0] = torch.tensor([1.0, 3.0, 3.0, 0.0, 3.0])             # tie of 1, 2, 4 -> 1
    lo[0, :, 0, 1] = 2.0                                                   # all equal -> 0
    lo[0, :, 0, 2] = torch.tensor([0.0, 9.0, float('nan'), 10.0, 1.0])     # NaN in one class -> 2
    lo[0, :, 0, 3] = torch.tensor([0.0, float('nan'), 50.0, float('nan'), 1.0])   # two NaN -> the first, 1
    lo[0, :, 1, 0] = torch.tensor([float('nan'), 1.0, 2.0, 3.0, 4.0])      # NaN in class 0 stays
    lo[0, :, 1, 1] = torch.tensor([-1.0, -1.0, -5.0, -1.0, -2.0])          # tie of the maximum among negatives -> 0
    y = torch.zeros(1, 4, 4, dtype=torch.uint8)
    cm, pred = ops.argmax_confusion(lo.to(DEV), y.to(DEV), Cc, None, 255, True, want_pred=True)
    want = lo.argmax(1)
    assert [int(want[0, 0, j]) for j in range(4)] == [1, 0, 2, 1] and int(want[0, 1, 0]) == 0 and int(want[0, 1, 1]) == 0
    assert torch.equal(pred.cpu().long(), want)
    assert np.array_equal(cm.cpu().numpy(), R.confusion(y.numpy(), want.numpy(), Cc, 255))


@pytest.mark.parametrize('Cc', [1, 5, 64])
def test_confusion_drops_out_of_range_predictions(ops, Cc):
    """hole 7: cms_confusion with predictions >= C (dropped), truth >= C and the ignore value; beyond 1024 x 256 elements"""
    rng = np.random.RandomState(Cc)
    n = 300000
    t = rng.randint(0, min(Cc + 3, 256), size=n).astype(np.uint8)
    p = rng.randint(0, min(Cc + 5, 256), size=n).astype(np.uint8)
    t[::11] = 255
    for ignore in (255, None, 0):
        cm = ops.confusion(torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV), Cc, ignore)
        assert np.array_equal(cm.cpu().numpy(), R.confusion(t, p, Cc, ignore))
    cm2 = ops.confusion(torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV), Cc, 255, cm=cm)
    assert np.array_equal(cm2.cpu().numpy(), R.confusion(t, p, Cc, 0) + R.confusion(t, p, Cc, 255))


# ====================================================================================================== NCHW upsample
_NCHW_CASES = [(g, 2, 3) for g in R.BILINEAR_GEOS] + [(R.NCHW_WRAP_FWD, 2, 8), (R.NCHW_WRAP_BWD, 2, 8)]


@pytest.mark.parametrize('align', [False, True], ids=['half_pixel', 'align_corners'])
@pytest.mark.parametrize('case', _NCHW_CASES, ids=lambda c: '{}x{}to{}x{}'.format(c[0][0][0], c[0][0][1], c[0][1][0], c[0][1][1]))
def test_upsample_bilinear_nchw_forward_and_backward(ops, case, align):
    """hole 8 (and 2): ops.upsample_bilinear (upsample_fwd_kernel, d = 3; upsample_bwd_kernel / footprint, d = touching output
    pixels) for both conventions at the geometry list of the NHWC kernels -- downsampling, size-1 sources and outputs included --
    plus one size whose forward (1 056 784 outputs) and one whose backward wraps the 4096-block grid."""
    ((h, w), (H, W)), N, Cc = case
    x = _randn((N, Cc, h, w), torch.float32, 1)
    dy = _randn((N, Cc, H, W), torch.float32, 2)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.upsample_bilinear(xd, (H, W), align_corners=align)
    out.backward(dy.to(DEV))
    tag = '{}x{}to{}x{} align={}'.format(h, w, H, W, int(align))
    ref, A = R.upsample_bilinear(_np(x), (H, W), align, 'nchw', W32)
    bf = R.bound(A, 3)
    R.assert_within(_np(out), ref, bf, 'upsample_nchw_fwd fp32 ' + tag)
    adj, Aa, d = R.upsample_bilinear_adjoint(_np(dy), (h, w), align, 'nchw', W32)
    ba = R.bound(Aa, d)
    R.assert_within(_np(xd.grad), adj, ba, 'upsample_nchw_bwd fp32 ' + tag)
    lhs, rhs = R.dot64(_np(out), _np(dy)), R.dot64(_np(x), _np(xd.grad))
    assert abs(lhs - rhs) <= float((bf * np.abs(_np(dy))).sum() + (ba * np.abs(_np(x))).sum()), (lhs, rhs)


# ====================================================================================================== optimizers
_SEG_SIZES = (1, 3, 4, 5, 2047, 2048, 2049, 6151)


class _Toy(torch.nn.Module):
    """fp32 state with segments of 1, 3, 4, 5, 2047, 2048, 2049 and 6151 elements (one 2048-element chunk and its neighbours, three
    chunks + a 7-element tail), a BatchNorm (two parameters, two buffers: k = 0 segments) and a frozen parameter"""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for n in _SEG_SIZES:
            setattr(self, 'p{}'.format(n), torch.nn.Parameter(torch.randn(n, generator=g)))
        self.bn = torch.nn.BatchNorm2d(6)
        with torch.no_grad():
            self.bn.weight.copy_(torch.rand(6, generator=g) + 0.5)
            self.bn.bias.copy_(torch.randn(6, generator=g))
            self.bn.running_mean.copy_(torch.randn(6, generator=g))
            self.bn.running_var.copy_(torch.rand(6, generator=g) + 0.5)
        self.frozen = torch.nn.Parameter(torch.randn(37, generator=g), requires_grad=False)


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('name', ['adam', 'sgd', 'sgd_nesterov'])
def test_fused_optimizer_segments_tails_padding_ema_and_shadows(name, grad_scale):
    """hole 9: three steps of FusedAdam / FusedSGD (+ nesterov) with an attached EMA teacher, bf16 shadows on both sides, two lr
    groups, parameters listed 3 and 4 times, a gradient scale, fresh gradients per step and a changed lr at step 3, against
    oracle/ema_opt.py per segment (tolerances of test_fused_optimizers_vs_golden). The gradient arena is random EVERYWHERE -- in the
    ALIGN padding and in the k = 0 segments too -- so a lane that strays past a segment's end shows. Exact: padding still zero,
    k = 0 segments bit-unchanged, teacher = ema_step(post-update student) bit for bit, bf16 shadows = RNE of their arenas."""
    from cutmix_semisup_seg_amd import optim as fo
    from cutmix_semisup_seg_amd import optim_weight_ema as fema
    from cutmix_semisup_seg_amd.arena import ensure_arena, ALIGN
    from oracle import ema_opt
    stu, tea = _Toy(1).to(DEV), _Toy(2).to(DEV)
    for p in tea.parameters():
        p.requires_grad = False
    sa, ta = ensure_arena(stu, with_grad=True, with_bf16=True), ensure_arena(tea, with_grad=False, with_bf16=True)
    lrs = [3e-3, 7e-4]
    g0 = [stu.p1, stu.p3, stu.p3, stu.p3, stu.p4, stu.p2047, stu.bn.weight]
    g1 = [stu.p5, stu.p2048, stu.p2048, stu.p2048, stu.p2048, stu.p2049, stu.p6151, stu.bn.bias]
    groups = [dict(params=g0, lr=lrs[0]), dict(params=g1, lr=lrs[1])]
    hyper = dict(momentum=0.9, nesterov=(name == 'sgd_nesterov'), weight_decay=5e-4)
    opt = fo.FusedAdam(stu, groups) if name == 'adam' else fo.FusedSGD(stu, groups, **hyper)
    alpha = 0.99
    ema = fema.EMAWeightOptimizer(tea, stu, alpha)
    ema.fuse_into(opt)
    opt.grad_scale = grad_scale
    assert sa.same_layout(ta) and sa.bf16 is not None and ta.bf16 is not None
    want_k = {'p1': 1, 'p3': 3, 'p4': 1, 'p5': 1, 'p2047': 1, 'p2048': 4, 'p2049': 1, 'p6151': 1, 'bn.weight': 1, 'bn.bias': 1,
              'bn.running_mean': 0, 'bn.running_var': 0, 'frozen': 0}
    assert dict(opt.k_updates) == want_k
    assert sorted(s.count for s in sa.segments) == sorted(_SEG_SIZES + (6, 6, 6, 6, 37))
    group_of = {id(p): gi for gi, grp in enumerate((g0, g1)) for p in grp}
    named = dict(stu.named_parameters())
    pad = np.ones(sa.total, dtype=bool)
    for s in sa.segments:
        pad[s.offset:s.offset + s.count] = False
    assert pad.sum() > 0 and sa.total % ALIGN == 0
    flat0 = sa.flat.cpu().numpy().copy()
    assert np.array_equal(ta.flat.cpu().numpy(), flat0)                       # the teacher starts as a copy
    ref_p = {s.key: flat0[s.offset:s.offset + s.count].copy() for s in sa.segments}
    ref_m = {s.key: (None if name != 'adam' else np.zeros(s.count, np.float32)) for s in sa.segments}
    ref_v = {s.key: np.zeros(s.count, np.float32) for s in sa.segments}
    tea_ref = flat0.copy()
    for step in range(3):
        if step == 2:
            lrs = [1.1e-3, 2.3e-4]
            for grp, lr in zip(opt.param_groups, lrs):
                grp['lr'] = lr
        opt.zero_grad()
        gen = torch.Generator().manual_seed(100 + step)
        grad = torch.randn(sa.total, generator=gen)
        sa.grad.copy_(grad.to(DEV))
        opt.step()
        ema.step()
        torch.cuda.synchronize()
        flat = sa.flat.cpu().numpy()
        gh = grad.numpy()
        for s in sa.segments:
            k = want_k[s.key]
            sl = slice(s.offset, s.offset + s.count)
            if k == 0:
                assert np.array_equal(flat[sl], flat0[sl]), s.key                # bit-unchanged
                continue
            lr = lrs[group_of[id(named[s.key])]]
            g = (gh[sl] * np.float32(grad_scale)).astype(np.float32)
            if name == 'adam':
                ref_p[s.key], ref_m[s.key], ref_v[s.key], _ = ema_opt.adam_k_updates(ref_p[s.key], g, ref_m[s.key], ref_v[s.key],
                                                                                     step * k, lr, k)
            else:
                ref_p[s.key], ref_m[s.key] = ema_opt.sgd_k_updates(ref_p[s.key], g, ref_m[s.key], lr, k, **hyper)
            np.testing.assert_allclose(flat[sl], ref_p[s.key], rtol=3e-6, atol=2e-7, err_msg=s.key)
        # teacher: the EMA of the student the kernel just wrote, three roundings, bit for bit -- every segment, buffers too
        tea_ref = np.where(pad, tea_ref, ema_opt.ema_step(tea_ref, flat, alpha))
        assert np.array_equal(ta.flat.cpu().numpy(), tea_ref)
        assert not flat[pad].any() and not ta.flat.cpu().numpy()[pad].any()
        assert torch.equal(sa.bf16, sa.flat.to(torch.bfloat16)) and torch.equal(ta.bf16, ta.flat.to(torch.bfloat16))
    assert int(opt.step_count) == 3
    s0 = opt.slot0.cpu().numpy()
    assert not s0[pad].any()
    if name == 'adam':
        s1 = opt.slot1.cpu().numpy()
        assert not s1[pad].any()
    for s in sa.segments:
        sl = slice(s.offset, s.offset + s.count)
        if want_k[s.key] == 0:
            assert not s0[sl].any()
        elif name == 'adam':
            np.testing.assert_allclose(s0[sl], ref_m[s.key], rtol=1e-5, atol=1e-8, err_msg=s.key)
            np.testing.assert_allclose(s1[sl], ref_v[s.key], rtol=1e-5, atol=1e-12, err_msg=s.key)
        else:
            np.testing.assert_allclose(s0[sl], ref_m[s.key], rtol=3e-6, atol=2e-7, err_msg=s.key)


# ====================================================================================================== all-ignored CE
@pytest.mark.parametrize('geo', [(2, 21, 41, 41, 321, 321, True), (2, 6, 9, 11, 40, 57, False)], ids=['C21_ac', 'C6_half_pixel'])
def test_ce_all_ignored_fused_gradient_is_zero(ops, geo):
    """hole 10: every supervised label ignored. The loss is NaN (0 / 0, as nn.CrossEntropyLoss gives); the gradient of ce_fused on its
    one-launch path (cms_ce_fwd_bwd, then the deferred factor) equals the ce_forward / ce_backward pair's, which is all zeros (the
    factor weight / 0 = inf must not meet the zero rows)."""
    from cutmix_semisup_seg_amd._lib import fn
    N, Cc, h, w, H, W, ac = geo
    lo = _randn((N, Cc, h, w), torch.float32, 1, 2.0).to(DEV)
    y = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
    sc2, ctx = ops.ce_forward(lo, y, (H, W), 255, ac)
    g2 = ops.ce_backward(ctx, sc2)
    assert torch.isnan(sc2[0]) and not bool(g2.any())
    assert bool(fn['cms_ce_fused_supported'](C.byref(ctx[0]))), 'this geometry must take the one-launch path'
    g1 = torch.zeros(N, Cc, h, w, device=DEV)
    sc1 = ops.ce_fused(lo, y, g1, (H, W), 255, ac)
    assert torch.isnan(sc1[0])
    assert torch.equal(g1, g2)
    # one label valid: the factor is finite again (weight / 1) and reaches the rows
    y[0, 3, 5] = 1
    g1.zero_()
    sc1 = ops.ce_fused(lo, y, g1, (H, W), 255, ac)
    assert bool(torch.isfinite(sc1).all()) and float(sc1[1]) == 1.0
    assert bool(torch.isfinite(g1).all()) and bool(g1.any())
