"""
Plain references for the stem convolution kernels of csrc/stem.hip (stem_fwd_kernel, stem_fwd_mfma_kernel, stem_wgrad_kernel,
stem_wgrad_mfma_kernel + stem_wgrad_reduce_kernel, stem_dgrad_kernel), written from the DEFINITION of the 7 x 7 / stride 2 / pad 3
convolution in numpy fp64 -- a loop over the 49 taps of the zero-padded image, no tiling, no grid -- plus the cases the CPU and the GPU
tests share. tests/test_stem_refs_cpu.py pins every function here against torch fp64 (F.conv2d and autograd) and checks that the bounds
the GPU tests assert would notice a dropped or a stale tile; tests/test_gpu_stem_kernels.py compares the kernels with them.

Conventions of tests/_stream_refs.py: every arithmetic reference returns (ref, A), A = the same expression on absolute values, and the
GPU tests assert |got - ref| <= (d + 2) * u32 * A [+ u_bf * |ref|] on every element (`_stream_refs.bound`), d stated at each use.

Layouts: image x (N, 3, H, W); activations and their gradients NHWC (N, Ho, Wo, 64); weights and their gradient in the arena's physical
(49, 64, 3) = [ky * 7 + kx][co][c].

The only facts about the LAUNCHES restated here are the ones a bound or a case needs and a test asserts against the library: the tile
sizes and block caps (`wgrad_plan`, `FWD_TILE`, `FWD_CAP`; the GPU test reads the block count back from
cms_stem_wgrad_workspace_bytes and compares).
"""
import collections

import numpy as np

from _stream_refs import bound

K, CO = 7, 64


def stem_out_hw(h, w):
    """(Ho, Wo) of the 7 x 7 / 2 / pad 3 convolution"""
    return (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1


def bf16_round(a):
    """fp32 -> the nearest bf16 value (ties to even), returned as fp32; finite inputs only"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def _padded(x):
    x = np.asarray(x, dtype=np.float64)
    return np.pad(x, ((0, 0), (0, 0), (3, 3), (3, 3)))


def _tap(P, ky, kx, ho, wo):
    """the input pixel every output pixel sees through tap (ky, kx): (N * Ho * Wo, 3)"""
    return np.ascontiguousarray(P[:, :, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2].transpose(0, 2, 3, 1)).reshape(-1, 3)


def _conv(x, w):
    n, _, h, wd = x.shape
    ho, wo = stem_out_hw(h, wd)
    P = _padded(x)
    out = np.zeros((n * ho * wo, CO))
    for ky in range(K):
        for kx in range(K):
            out += _tap(P, ky, kx, ho, wo) @ w[ky * K + kx].T              # sum over c of x[c] * w[co][c]
    return out.reshape(n, ho, wo, CO)


def stem_forward(x, w, scale, bias):
    """relu(conv7x7/2/pad3(x, w) * scale + bias) as NHWC -> (ref, A), A = (|x| conv |w|) * |scale| + |bias| (the bound of the value
    before the ReLU, which does not increase an error)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    scale, bias = np.asarray(scale, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    ref = np.maximum(_conv(x, w) * scale + bias, 0.0)
    return ref, _conv(np.abs(x), np.abs(w)) * np.abs(scale) + np.abs(bias)


def _wgrad(x, ds):
    n, ho, wo, _ = ds.shape
    assert (ho, wo) == stem_out_hw(x.shape[2], x.shape[3])
    P = _padded(x)
    d2 = ds.reshape(-1, CO)
    dw = np.zeros((K * K, CO, 3))
    for ky in range(K):
        for kx in range(K):
            dw[ky * K + kx] = d2.T @ _tap(P, ky, kx, ho, wo)               # sum over the pixels of dS[co] * x[c]
    return dw


def stem_wgrad(x, ds, scale=None):
    """dW[ky * 7 + kx][co][c] = scale[co] * sum_{n, oy, ox} dS[n, oy, ox, co] * x[n, c, 2 oy - 3 + ky, 2 ox - 3 + kx] -> (ref, A);
    scale None = 1 (the bn_trainable path)."""
    x, ds = np.asarray(x, dtype=np.float64), np.asarray(ds, dtype=np.float64)
    return scaled(_wgrad(x, ds), _wgrad(np.abs(x), np.abs(ds)), scale)


def scaled(ref, A, scale):
    """(ref, A) of stem_wgrad(..., None) -> (ref, A) with a per-channel scale (so the sums are computed once for both)"""
    if scale is None:
        return ref, A
    s = np.asarray(scale, dtype=np.float64).reshape(1, CO, 1)
    return ref * s, A * np.abs(s)


def _dgrad(g, w, hw):
    # g (N, Ho, Wo, 64) already times scale
    n, ho, wo, _ = g.shape
    h, wd = hw
    assert (ho, wo) == stem_out_hw(h, wd)
    D = np.zeros((n, 3, h + 6, wd + 6))
    g2 = g.reshape(-1, CO)
    for ky in range(K):
        for kx in range(K):
            D[:, :, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] += (g2 @ w[ky * K + kx]).reshape(n, ho, wo, 3).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(D[:, :, 3:3 + h, 3:3 + wd])


def stem_dgrad(ds, w, scale, hw):
    """dx[n, c, iy, ix] = sum over (ky, kx, co) with 2 oy - 3 + ky = iy, 2 ox - 3 + kx = ix of dS[n, oy, ox, co] * scale[co] *
    w[ky * 7 + kx][co][c] -> (ref, A, taps): taps (H, W) = the number of (ky, kx) that reach an output pixel, per image pixel."""
    ds, w = np.asarray(ds, dtype=np.float64), np.asarray(w, dtype=np.float64)
    s = np.asarray(scale, dtype=np.float64)
    ho, wo = ds.shape[1:3]
    ones = np.zeros((1, ho, wo, CO))
    ones[..., 0] = 1.0
    sel = np.zeros((K * K, CO, 3))
    sel[:, 0, 0] = 1.0
    taps = np.rint(_dgrad(ones, sel, hw)[0, 0]).astype(np.int64)
    return _dgrad(ds * s, w, hw), _dgrad(np.abs(ds * s), np.abs(w), hw), taps


# ------------------------------------------------------------------------------------------------------------ launches
FWD_TILE = (16, 16)          # stem_fwd_kernel / stem_fwd_mfma_kernel / stem_wgrad_mfma_kernel: output tile
FWD_CAP = 512                # persistent workgroups of stem_fwd_mfma_kernel
VALU_WGRAD_TILE = (8, 16)    # stem_wgrad_kernel
WGRAD_CAP = {True: 256, False: 768}

Plan = collections.namedtuple('Plan', 'mfma tile tiles_y tiles_x ntiles nblocks pixels')


def n_tiles(n, h, w, tile):
    ho, wo = stem_out_hw(h, w)
    return n * (-(-ho // tile[0])) * (-(-wo // tile[1]))


def wgrad_plan(x_bf16, ds_bf16, n, h, w):
    """which weight-gradient kernel a type pair runs (matrix cores only for bf16 x bf16) and how its tiles are dealt"""
    mfma = bool(x_bf16 and ds_bf16)
    tile = FWD_TILE if mfma else VALU_WGRAD_TILE
    ho, wo = stem_out_hw(h, w)
    ty, tx = -(-ho // tile[0]), -(-wo // tile[1])
    nt = n * ty * tx
    return Plan(mfma, tile, ty, tx, nt, min(nt, WGRAD_CAP[mfma]), tile[0] * tile[1])


def wgrad_depth(plan, calls=1):
    """longest chain of fp32 additions behind one element of dW, read off the kernels: a block's accumulator takes one addition per
    pixel of each of its ceil(ntiles / nblocks) tiles (128 VALU, 256 on the matrix cores: 4 stages x 4 MFMAs of 16 pixels), then
    the element takes one addition per block -- the atomics in any order, or the ordered combine of the slabs, whose chain
    (nblocks / 16 + 5) is shorter -- and that once per call accumulated into the same buffer."""
    return -(-plan.ntiles // plan.nblocks) * plan.pixels + calls * plan.nblocks


def wgrad_bound(A, fill, plan, calls=1):
    """bound of `calls` launches accumulated into a buffer pre-filled with `fill`: the reference is fill + calls * ref, its sum of
    absolute values |fill| + calls * A"""
    return bound(abs(fill) + calls * np.asarray(A), wgrad_depth(plan, calls))


def tile_of(t, plan):
    """tile index -> (image, first output row, first output column): the kernels' own enumeration, x fastest"""
    return t // (plan.tiles_x * plan.tiles_y), (t // plan.tiles_x) % plan.tiles_y * plan.tile[0], t % plan.tiles_x * plan.tile[1]


def drop_tile(x, ds, scale, ref, t, plan):
    """the weight-gradient reference `ref` with the contribution of output tile `t` (of its one image) removed: what a kernel that
    skips that tile would have to produce. -> (reference, number of pixels dropped)"""
    n, oy, ox = tile_of(t, plan)
    only = np.zeros((1,) + tuple(ds.shape[1:]))
    cut = ds[n, oy:oy + plan.tile[0], ox:ox + plan.tile[1]]
    only[0, oy:oy + plan.tile[0], ox:ox + plan.tile[1]] = cut
    part, _ = stem_wgrad(x[n:n + 1], only, scale)
    return ref - part, cut.shape[0] * cut.shape[1]


def stale_tile_forward(x, w, scale, bias, ref, t, t_prev):
    """the forward reference `ref` with output tile `t` computed from the input patch of tile `t_prev` (the tile the same persistent
    workgroup took one trip earlier): what stem_fwd_mfma_kernel stores when a tile is computed before its patch has replaced the
    previous one in LDS."""
    n, ho, wo, _ = ref.shape
    ty, tx = -(-ho // FWD_TILE[0]), -(-wo // FWD_TILE[1])
    plan = Plan(True, FWD_TILE, ty, tx, n * ty * tx, 0, 256)
    (n1, oy1, ox1), (n0, oy0, ox0) = tile_of(t, plan), tile_of(t_prev, plan)
    th, tw = min(FWD_TILE[0], ho - oy1), min(FWD_TILE[1], wo - ox1)
    # the 37 x 37 patch of t_prev, zero outside the image like the kernel's staging loop, as an image of its own whose convolution
    # WITHOUT padding is the 16 x 16 tile
    P = _padded(np.asarray(x, dtype=np.float64)[n0:n0 + 1])
    patch = np.zeros((1, 3, 37, 37))
    src = P[:, :, 2 * oy0:2 * oy0 + 37, 2 * ox0:2 * ox0 + 37]
    patch[:, :, :src.shape[2], :src.shape[3]] = src
    w = np.asarray(w, dtype=np.float64)
    tile = np.zeros((16, 16, CO))
    for ky in range(K):
        for kx in range(K):
            tile += np.einsum('cyx,oc->yxo', patch[0, :, ky:ky + 31:2, kx:kx + 31:2], w[ky * K + kx])
    out = ref.copy()
    out[n1, oy1:oy1 + th, ox1:ox1 + tw] = np.maximum(tile[:th, :tw] * np.asarray(scale, dtype=np.float64) + np.asarray(bias, dtype=np.float64), 0.0)
    return out


def forward_bound(A, ref, bf16_out, mfma):
    """VALU kernel: 147 fused multiply-adds in one chain, then the scale product and the bias addition (d = 147, the "+ 2").
    Matrix-core kernel: the same plus 2^-16 * A -- the fp32 weight enters as a bf16 pair hi + lo, hi = bf16(w), lo = bf16(w - hi):
    |w - hi| <= 2^-8 |w| (one bf16 ulp; half of it with round-to-nearest) and lo is rounded to bf16 in turn, relative 2^-9 (half an
    ulp), so |w - (hi + lo)| <= 2^-9 * 2^-8 |w|, counted once for each of the two products (hi * x and lo * x) that replace w * x.
    Its 22 MFMAs of 16 products each (two (c, ky) rows of 8 per step, hi and lo) form a chain no longer than the VALU kernel's."""
    b = bound(A, 147, ref, bf16_out)
    return b + 2.0 ** -16 * np.asarray(A) if mfma else b


def dgrad_bound(A, taps):
    """stem_dgrad_kernel: one thread per image pixel, one chain of 64 fused multiply-adds per contributing tap, each operand
    dS * scale rounded once (d = 64 * taps + 2; bound adds its own 2 for the product roundings)"""
    return bound(A, 64.0 * taps[None, None] + 2.0)


# ------------------------------------------------------------------------------------------------------------ cases
# dist 'signed':   x ~ N(0, 1), dS ~ N(0, 1) with half of the elements exactly zero (the ReLU gate) -- cancelling sums, A >> |ref|
# dist 'positive': x = 1 + N(0, 1) / 4, dS = U[0.5, 1.5) on 1 / 16 of the elements, else 0 (sparse like the gradient behind the
#                  max-pool, non-negative) -- nothing cancels in the weight gradient, A ~ |ref|, and one pixel carries 16 / P of a
#                  channel's sum instead of 1 / P: the condition under which the weight-gradient bound notices ONE dropped tile
#                  of the persistent case, down to the 1-pixel corner tile of the 8 x 16 tiling (tests/test_stem_refs_cpu.py
#                  asserts that it does)
Case = collections.namedtuple('Case', 'name n h w dist seed')
PERSISTENT = Case('persistent', 66, 49, 97, 'positive', 101)
EDGES = [Case('1x1', 2, 1, 1, 'signed', 102), Case('5x40', 1, 5, 40, 'signed', 103), Case('8x6', 2, 8, 6, 'signed', 104),
         Case('16x34', 1, 16, 34, 'signed', 105), Case('33x47', 3, 33, 47, 'signed', 106)]
REDUCE = [Case('reduce{}'.format(n), n, 9, 9, 'signed', 110 + n) for n in (1, 3, 5, 13, 17)]
CASES = [PERSISTENT] + EDGES + REDUCE
PREFILL = 0.25               # the weight-gradient buffer is accumulated into: its content before the launch

Inputs = collections.namedtuple('Inputs', 'x ds w scale bias')


def case_inputs(case, n=None):
    """fp32 inputs of a case (numpy); `n` = a smaller batch of the same distribution (CPU pins). Weights are fp32 numbers that bf16
    cannot hold; `to_bf16` makes the bf16-exact variant of an image / gradient."""
    n = case.n if n is None else n
    rng = np.random.RandomState(case.seed)
    ho, wo = stem_out_hw(case.h, case.w)
    if case.dist == 'positive':
        x = 1.0 + rng.randn(n, 3, case.h, case.w) / 4.0
        ds = (0.5 + rng.rand(n, ho, wo, CO)) * (rng.rand(n, ho, wo, CO) < 1.0 / 16.0)
    else:
        x = rng.randn(n, 3, case.h, case.w)
        ds = rng.randn(n, ho, wo, CO) * (rng.rand(n, ho, wo, CO) > 0.5)
    w = rng.randn(K * K, CO, 3) * 0.1
    scale, bias = rng.rand(CO) + 0.5, rng.randn(CO) * 0.2
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return Inputs(f(x), f(ds), f(w), f(scale), f(bias))


def typed(a, bf16):
    return bf16_round(a) if bf16 else a
