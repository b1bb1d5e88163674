"""
Plain references for the bandwidth-bound kernels (csrc/nhwc.hip, aspp.hip, upsample.hip, eval.hip, the max-pool of stem.hip),
written from each operation's DEFINITION in numpy fp64 -- no tiling, no grid, no unrolling -- plus the error-bound helpers the GPU
tests assert with. tests/test_stream_refs_cpu.py pins every function here against torch in fp64 on the CPU, so the GPU tests can
trust them; tests/test_gpu_stream_kernels.py compares the kernels with them.

Every reference of an arithmetic operation returns (ref, A): the value in fp64 and the same expression evaluated on absolute
values, A = sum |w| * |v|, the scale of the rounding-error bound

    |got - ref| <= (d + 2) * u32 * A  [+ u_bf * |ref| when the result is stored as bf16]            (`bound`)

for a sum of products accumulated in fp32 whose longest chain of additions has depth d (u32 = 2^-24, u_bf = 2^-8). The "+ 2" pays
for the rounding of a weight product and of a final scale factor. bf16 / fp32 inputs are exact in fp64, so reference and kernel
start from the same bits.

Bilinear weights. F.interpolate computes the source coordinate and the two weights of an output index in the tensor's own
precision: for fp32 tensors they ARE fp32 numbers (scale = in / out, src = fma(scale, dst + 0.5, -0.5), lambda = src - floor(src),
each operation rounded once). `weight_dtype=np.float32` restates exactly that (pinned bit for bit against torch's fp32 weights on
the CPU); the interpolation itself is then done in fp64 with those weights. This is the reference the fp32 kernels are held to:
a reference with fp64 weights differs from ANY fp32 implementation of the definition by ~ u32 * src in lambda, which is a
property of the operation's definition in fp32 and not an accumulation error of a kernel. `weight_dtype=np.float64` is the same
definition in fp64 (pinned against torch fp64).
"""
import numpy as np

U32 = 2.0 ** -24
UBF = 2.0 ** -8


# ------------------------------------------------------------------------------------------------------------ bounds
def bound(A, d, ref=None, bf16_out=False):
    """(d + 2) * u32 * A [+ u_bf * |ref|]: element-wise; `d` a number or an array like A."""
    b = (np.asarray(d, dtype=np.float64) + 2.0) * U32 * np.asarray(A, dtype=np.float64)
    if bf16_out:
        b = b + UBF * np.abs(ref)
    return b


def worst_ratio(got, ref, bnd):
    """max over ALL elements of |got - ref| / bound (0 / 0 = 0: an exact element with a zero bound is fine, a wrong one is inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / bnd)
    return float(r.max()) if r.size else 0.0


def assert_within(got, ref, bnd, what=''):
    """element-wise over all elements, no exclusions; prints the largest |got - ref| / bound before asserting"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what + ': non-finite output'
    r = worst_ratio(got, ref, bnd)
    print('RATIO {} {:.4f}'.format(what, r))
    if not r <= 1.0:
        err = np.abs(got - ref)
        bad = np.argwhere(err > bnd)
        i = tuple(bad[0])
        raise AssertionError('{}: {} of {} elements beyond the bound, worst |err| / bound = {:.3f}; first at {}: got {!r} ref {!r} '
                             'bound {!r}'.format(what, len(bad), err.size, r, i, got[i], ref[i], np.broadcast_to(bnd, err.shape)[i]))
    return r


def dot64(a, b):
    return float(np.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------------------ bilinear
def bilinear_taps(in_size, out_size, align_corners, weight_dtype=np.float64):
    """F.interpolate(mode='bilinear') along one axis: (i0, i1, w0, w1) per output index, arithmetic in `weight_dtype`."""
    T = weight_dtype
    dst = np.arange(out_size).astype(T)
    if align_corners:
        scale = T(in_size - 1) / T(out_size - 1) if out_size > 1 else T(0)
        src = (scale * dst).astype(T)
    else:
        scale = T(in_size) / T(out_size)
        if T is np.float64:
            src = scale * (dst + T(0.5)) - T(0.5)
        else:
            # one rounding: scale * (dst + 0.5) - 0.5 is a fused multiply-add in torch's compiled kernels (the product of two fp32
            # numbers is exact in fp64, so is the difference here; the cast rounds once)
            src = (np.float64(scale) * (dst + T(0.5)).astype(np.float64) - 0.5).astype(T)
        src = np.maximum(src, T(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    lam = np.clip((src - i0.astype(T)).astype(T), T(0), T(1))
    w1 = lam.astype(T)
    w0 = (T(1) - lam).astype(T)
    return i0, i1, w0, w1


def bilinear_matrix(in_size, out_size, align_corners, weight_dtype=np.float64):
    """(out, in) fp64 matrix of the 1-D interpolation and the number of non-zero entries per COLUMN (taps of the adjoint)."""
    i0, i1, w0, w1 = bilinear_taps(in_size, out_size, align_corners, weight_dtype)
    M = np.zeros((out_size, in_size), dtype=np.float64)
    r = np.arange(out_size)
    np.add.at(M, (r, i0), w0.astype(np.float64))
    np.add.at(M, (r, i1), w1.astype(np.float64))
    return M, (M != 0.0).sum(axis=0)


def _apply2(My, Mx, x, layout):
    # x: (N, h, w, C) 'nhwc' or (N, C, h, w) 'nchw'; rows by My (H, h), columns by Mx (W, w)
    if layout == 'nhwc':
        return np.einsum('Yy,nyXc->nYXc', My, np.einsum('Xx,nyxc->nyXc', Mx, x, optimize=True), optimize=True)
    return np.einsum('Yy,ncyX->ncYX', My, np.einsum('Xx,ncyx->ncyX', Mx, x, optimize=True), optimize=True)


def upsample_bilinear(x, size, align_corners, layout='nhwc', weight_dtype=np.float64):
    """-> (ref, A). x fp64 (N, h, w, C) or (N, C, h, w). Depth of the addition chain: d = 3 (four products)."""
    x = np.asarray(x, dtype=np.float64)
    h, w = (x.shape[1], x.shape[2]) if layout == 'nhwc' else (x.shape[2], x.shape[3])
    My, _ = bilinear_matrix(h, size[0], align_corners, weight_dtype)
    Mx, _ = bilinear_matrix(w, size[1], align_corners, weight_dtype)
    return _apply2(My, Mx, x, layout), _apply2(My, Mx, np.abs(x), layout)


def upsample_bilinear_adjoint(g, in_hw, align_corners, layout='nhwc', weight_dtype=np.float64):
    """Exact adjoint U^T g of the map above -> (ref, A, d): d (h, w) = number of output pixels that touch each source pixel."""
    g = np.asarray(g, dtype=np.float64)
    H, W = (g.shape[1], g.shape[2]) if layout == 'nhwc' else (g.shape[2], g.shape[3])
    My, cy = bilinear_matrix(in_hw[0], H, align_corners, weight_dtype)
    Mx, cx = bilinear_matrix(in_hw[1], W, align_corners, weight_dtype)
    d = np.outer(cy, cx).astype(np.float64)
    d = d[None, :, :, None] if layout == 'nhwc' else d[None, None, :, :]
    return _apply2(My.T.copy(), Mx.T.copy(), g, layout), _apply2(My.T.copy(), Mx.T.copy(), np.abs(g), layout), d


# ------------------------------------------------------------------------------------------------------------ concat / sums
def concat_broadcast(xs):
    """channel concat of NHWC arrays; (N, 1, 1, C) inputs are broadcast over the map of the others."""
    big = next((x for x in xs if x.shape[1] * x.shape[2] > 1), xs[0])
    n, h, w = big.shape[:3]
    return np.concatenate([np.broadcast_to(x, (n, h, w, x.shape[3])) for x in xs], axis=3)


def concat_broadcast_adjoint(g, shapes):
    """-> [(ref, A)] per input: the channel slice, summed over the pixels for a broadcast input (A = the sum of |g|)."""
    g = np.asarray(g, dtype=np.float64)
    out, off = [], 0
    for s in shapes:
        sl = g[..., off:off + s[3]]
        off += s[3]
        if tuple(s[1:3]) == (1, 1) and sl.shape[1:3] != (1, 1):
            out.append((sl.sum(axis=(1, 2), keepdims=True), np.abs(sl).sum(axis=(1, 2), keepdims=True)))
        else:
            out.append((sl.copy(), np.abs(sl)))
    return out


def mean_over_pixels(x):
    """(N, H, W, C) -> (ref, A) of shape (N, 1, 1, C)"""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[1] * x.shape[2]
    return x.sum(axis=(1, 2), keepdims=True) / rows, np.abs(x).sum(axis=(1, 2), keepdims=True) / rows


def sum_k(xs):
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    return sum(xs[1:], xs[0].copy()), sum((np.abs(x) for x in xs[1:]), np.abs(xs[0]))


def rows_reduce_depth(rows):
    """32 row slots side by side, each a serial chain of ceil(rows / 32) additions, then a serial sum over the 32 slots"""
    return -(-int(rows) // 32) + 32


# ------------------------------------------------------------------------------------------------------------ ASPP
def aspp_gather(z, bias, taps, C):
    """logits[n,c,y,x] = bias[c] + sum_k z[n, k*C + c, y + dy_k, x + dx_k] (zero outside the map) -> (ref, A)"""
    z = np.asarray(z, dtype=np.float64)
    n, zc, h, w = z.shape
    ref = np.zeros((n, C, h, w))
    A = np.zeros((n, C, h, w))
    if bias is not None:
        ref += np.asarray(bias, dtype=np.float64).reshape(1, C, 1, 1)
        A += np.abs(np.asarray(bias, dtype=np.float64)).reshape(1, C, 1, 1)
    for k, (dy, dx) in enumerate(taps):
        y0, y1 = max(0, -dy), min(h, h - dy)
        x0, x1 = max(0, -dx), min(w, w - dx)
        if y0 >= y1 or x0 >= x1:
            continue
        src = z[:, k * C:(k + 1) * C, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ref[:, :, y0:y1, x0:x1] += src
        A[:, :, y0:y1, x0:x1] += np.abs(src)
    return ref, A


def aspp_spread(dl, taps, zc):
    """D[n,y,x,k*C + c] = dl[n,c,y - dy_k,x - dx_k] (zero outside, zero in the columns >= T*C): pure data movement"""
    dl = np.asarray(dl)
    n, C, h, w = dl.shape
    D = np.zeros((n, h, w, zc), dtype=dl.dtype)
    for k, (dy, dx) in enumerate(taps):
        y0, y1 = max(0, dy), min(h, h + dy)
        x0, x1 = max(0, dx), min(w, w + dx)
        if y0 >= y1 or x0 >= x1:
            continue
        D[:, y0:y1, x0:x1, k * C:(k + 1) * C] = dl[:, :, y0 - dy:y1 - dy, x0 - dx:x1 - dx].transpose(0, 2, 3, 1)
    return D


# ------------------------------------------------------------------------------------------------------------ max-pool
def pool_out_size(s, ceil_mode):
    """kernel 3, stride 2, padding 1; in ceil mode the last window must start inside the input or its left padding"""
    if not ceil_mode:
        return (s + 2 - 3) // 2 + 1
    o = -(-(s + 2 - 3) // 2) + 1
    if (o - 1) * 2 >= s + 1:
        o -= 1
    return o


def _pool_padded(s, hp, wp, fill):
    n, hs, ws, c = s.shape
    P = np.full((n, 2 * hp + 1, 2 * wp + 1, c), fill, dtype=s.dtype)
    P[:, 1:1 + hs, 1:1 + ws, :] = s[:, :2 * hp, :2 * wp, :]
    return P


def maxpool3x3s2(s, ceil_mode):
    """NHWC -> window maxima (N, hp, wp, C); padding counts as -inf"""
    n, hs, ws, c = s.shape
    hp, wp = pool_out_size(hs, ceil_mode), pool_out_size(ws, ceil_mode)
    P = _pool_padded(s, hp, wp, -np.inf)
    out = np.full((n, hp, wp, c), -np.inf, dtype=s.dtype)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, P[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :])
    return out


def maxpool_window_value(s, idx, ceil_mode):
    """the element idx = ky * 3 + kx points at in each window, and whether it lies inside the input"""
    n, hs, ws, c = s.shape
    hp, wp = idx.shape[1:3]
    P = _pool_padded(s, hp, wp, -np.inf)
    inside = _pool_padded(np.ones(s.shape, dtype=bool), hp, wp, False)
    val = np.full(idx.shape, np.nan, dtype=s.dtype)
    ok = np.zeros(idx.shape, dtype=bool)
    for ky in range(3):
        for kx in range(3):
            m = idx == ky * 3 + kx
            val = np.where(m, P[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :], val)
            ok |= m & inside[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :]
    return val, ok


def maxpool3x3s2_relu_backward(dp, idx, s):
    """ds[n, 2py - 1 + ky, 2px - 1 + kx, c] += dp[n,py,px,c] for idx[n,py,px,c] = ky * 3 + kx, then gated by s > 0. The routing
    follows the GIVEN index map, so the result does not depend on how ties were broken."""
    dp = np.asarray(dp, dtype=np.float64)
    n, hs, ws, c = s.shape
    hp, wp = idx.shape[1:3]
    G = np.zeros((n, 2 * hp + 1, 2 * wp + 1, c))
    for ky in range(3):
        for kx in range(3):
            G[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :] += np.where(idx == ky * 3 + kx, dp, 0.0)
    ds = np.zeros((n, hs, ws, c))
    hh, ww = min(hs, 2 * hp), min(ws, 2 * wp)
    ds[:, :hh, :ww, :] = G[:, 1:1 + hh, 1:1 + ww, :]
    return np.where(np.asarray(s, dtype=np.float64) > 0, ds, 0.0)


# ------------------------------------------------------------------------------------------------------------ evaluation
def confusion(truth, pred, C, ignore_index=None):
    """(C, C) int64 counts, row = truth, column = prediction; truth outside [0, C) or equal to ignore_index and predictions
    >= C are dropped."""
    t = np.asarray(truth).astype(np.int64).ravel()
    p = np.asarray(pred).astype(np.int64).ravel()
    keep = (t >= 0) & (t < C) & (p >= 0) & (p < C)
    if ignore_index is not None:
        keep &= t != ignore_index
    return np.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C).astype(np.int64)


def argmax_margin(up):
    """(N, C, H, W) fp64 -> (top-1 class [first index on ties], top1 - top2 [inf for C = 1])"""
    top = up.argmax(axis=1)
    if up.shape[1] == 1:
        return top, np.full(top.shape, np.inf)
    srt = np.sort(up, axis=1)
    return top, srt[:, -1] - srt[:, -2]


# ------------------------------------------------------------------------------------------------------------ shared cases
# (h, w) -> (H, W) of the bilinear tests: size-1 sources and outputs, non-integer ratios both ways, ratios above 4
BILINEAR_GEOS = [((1, 1), (9, 7)), ((1, 5), (4, 20)), ((5, 1), (20, 3)), ((9, 9), (1, 1)), ((7, 5), (1, 9)), ((33, 33), (129, 129)),
                 ((17, 23), (65, 41)), ((65, 41), (17, 23)), ((40, 57), (13, 100)), ((3, 3), (50, 50))]
# grid-wrapping extras: nhwc adjoint with N * h * w * C / 8 > 1 048 576 work items; NCHW forward / backward beyond 4096 x 256
NHWC_WRAP_GEO = ((129, 129), (33, 33))          # N = 2, C = 256: 1 064 992 adjoint work items
NCHW_WRAP_FWD = ((33, 33), (257, 257))          # N * C = 16: 1 056 784 outputs
NCHW_WRAP_BWD = ((257, 257), (65, 65))          # N * C = 16: 1 056 784 source pixels
POOL_SHAPES = [(1, 1, 1, 8), (1, 2, 3, 8), (2, 7, 10, 16), (1, 12, 9, 24), (1, 161, 161, 64), (2, 257, 513, 128)]
ASPP_MAPS = [(1, 1, 1), (2, 5, 7), (1, 41, 41), (4, 65, 129)]
ASPP_CLASSES = [2, 5, 19, 21]
# argmax_confusion: (N, C, h, w, H, W, align_corners, seed); the last one has P > 1024 * 256
EVAL_CASES = [(2, 21, 41, 41, 161, 161, True, 11), (2, 21, 41, 41, 161, 161, False, 12), (1, 2, 9, 11, 40, 57, False, 13),
              (1, 64, 17, 17, 65, 65, True, 14), (3, 1, 5, 5, 9, 9, True, 15), (1, 21, 65, 129, 513, 1025, True, 16),
              (2, 21, 33, 47, 33, 47, True, 17)]
EVAL_LOGIT_SCALE = 2.0


def pool_input(shape, seed):
    """quarter-integer values: exact in bf16, full of exact ties and exact zeros (the s > 0 gate)"""
    rng = np.random.RandomState(seed)
    return (np.round(rng.randn(*shape) * 4.0) / 4.0).astype(np.float32)


def eval_logits(case):
    n, c, h, w = case[:4]
    return (np.random.RandomState(case[7]).randn(n, c, h, w) * EVAL_LOGIT_SCALE).astype(np.float32)
