"""
Plain references for the fp32 convolution family of csrc/conv_f32.hip (conv_f32_kernel in forward and data-gradient mode,
conv_wgrad_f32_kernel, pack_transpose_f32_kernel), written from the DEFINITIONS in numpy fp64 -- a loop over the taps, no tiling, no
knowledge of the kernels' layout -- plus the cases the CPU and the GPU tests share and the mutations the bounds must notice.
tests/test_conv_f32_refs_cpu.py pins every function here against torch fp64 (F.conv2d and autograd), asserts that every case lands on
the tile / split / slice its name says, and that the five mutations lie outside the bounds; tests/test_gpu_conv_f32_kernels.py compares
the kernels with them on every element.

Conventions of tests/_stream_refs.py: every arithmetic reference returns (ref, A), A = the same expression on absolute values (|scale|,
|bias|, |res|, |prefill| included); a gated element (mask <= 0) and a gradient row the launch must not write have A = 0: the bound there
is zero, the value must be exact.

Layouts: activations and their gradients NHWC (N, H, W, C); weights (taps, Cout, Cin); taps = [(dy, dx)] input offsets,
y[n, oy, ox, co] = sum_t sum_ci x[n, oy * stride + dy_t, ox * stride + dx_t, ci] * w[t, co, ci], zero outside the map.

BOUNDS. |got - ref| <= (d + 2) * u32 * A on every element (`_stream_refs.bound`, u32 = 2^-24), derived, not tuned:

  A sum of n products accumulated in fp32 IN ANY ORDER -- a chain, a tree, the MFMA's own order of K, partial sums combined by atomics --
  has |fl(sum) - sum| <= gamma_n * sum |a_i b_i|, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, section 3.1: each term
  passes through at most n roundings, one of its product and at most n - 1 additions; with fused multiply-adds fewer). So d only has to
  count the terms behind one element and does not depend on how the matrix cores order them. "+ 2" is the slack of `bound` (it pays for
  gamma_n against n u at these sizes: n u < 2^-12).

  forward / data gradient   d = (taps in the split) * Cin                       terms one workgroup accumulates for the element; taps
                                + (number of splits, when ksplit > 1)           outside the map count (zeros are terms too: upper bound)
                                + 1 per epilogue operand (scale, bias, res)     the atomics that combine the splits, one addition each
                            every operand is one more rounding of a value bounded by A. ReLU is 1-Lipschitz, the mask gate is an input:
                            neither adds an error nor excludes an element.
  weight gradient           d = (pixels per slice) + (number of slices)         a workgroup accumulates one slice of the pixel axis, then
                            A = |prefill| + |scale| * sum |dU| |x|              the element takes one atomic addition per slice, the
                                                                                first onto the buffer's content; the scale product is
                                                                                in the "+ 2". Same form as _stem_refs.wgrad_bound.
  re-pack                   none: one fp32 product per element -> compared bit for bit with the same product in np.float32.

The only facts about the LAUNCHES restated here are the ones a bound or a case needs (`fwd_plan`, `wgrad_plan`, read from
cms_conv_igemm_f32 / cms_conv_wgrad_f32); the CPU test asserts each case against them.
"""
import collections

import numpy as np

from _stream_refs import bound


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def conv_taps(k, dil, pad):
    """(dy, dx) of the k x k taps in [ky][kx] order"""
    return [(ky * dil - pad, kx * dil - pad) for ky in range(k) for kx in range(k)]


def conv_out(size, k, dil, pad, stride):
    return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _tap_window(t, taps, stride, in_hw, out_hw):
    """output rows / columns whose input through tap t lies inside the map, and those input rows / columns"""
    dy, dx = taps[t]
    iy, ix = np.arange(out_hw[0]) * stride + dy, np.arange(out_hw[1]) * stride + dx
    ys, xs = np.nonzero((iy >= 0) & (iy < in_hw[0]))[0], np.nonzero((ix >= 0) & (ix < in_hw[1]))[0]
    return ys, xs, iy[ys], ix[xs]


def conv(x, w, taps, stride=1, out_hw=None):
    """the bare sum over taps and input channels -> (N, Ho, Wo, Cout) fp64"""
    x, w = _f64(x), _f64(w)
    n, h, wd, cin = x.shape
    assert w.shape[0] == len(taps) and w.shape[2] == cin
    ho, wo = (h, wd) if out_hw is None else out_hw
    out = np.zeros((n, ho, wo, w.shape[1]))
    for t in range(len(taps)):
        ys, xs, iy, ix = _tap_window(t, taps, stride, (h, wd), (ho, wo))
        if ys.size == 0 or xs.size == 0:
            continue
        out[np.ix_(np.arange(n), ys, xs)] += x[:, iy][:, :, ix] @ w[t].T
    return out


def epilogue(acc, Aacc, scale=None, bias=None, res=None, relu=False):
    """acc * scale + bias + res, then ReLU -> (ref, A)"""
    ref, A = acc.copy(), Aacc.copy()
    if scale is not None:
        ref, A = ref * _f64(scale), A * np.abs(_f64(scale))
    if bias is not None:
        ref, A = ref + _f64(bias), A + np.abs(_f64(bias))
    if res is not None:
        ref, A = ref + _f64(res), A + np.abs(_f64(res))
    if relu:
        ref = np.maximum(ref, 0.0)
    return ref, A


def forward(x_nhwc, w_tap_co_ci, taps, stride=1, out_hw=None, scale=None, bias=None, res=None, relu=False):
    """relu?(conv(x, w) * scale + bias + res) as NHWC -> (ref, A)"""
    acc = conv(x_nhwc, w_tap_co_ci, taps, stride, out_hw)
    Aacc = conv(np.abs(_f64(x_nhwc)), np.abs(_f64(w_tap_co_ci)), taps, stride, out_hw)
    return epilogue(acc, Aacc, scale, bias, res, relu)


def nchw(a, cout_real=None):
    """NHWC -> the NCHW form with the first `cout_real` channels (the fp32 NCHW output of the head)"""
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2)[:, :cout_real])


def scatter_pixels(n, hw, out_full_hw, out_stride, out_pixel_offset):
    """flat pixel index in an (N, out_H, out_W) map of every result pixel (n, oy, ox) of an (N,) + hw launch:
    (n * out_H + oy * out_stride) * out_W + ox * out_stride + out_pixel_offset"""
    nn, oy, ox = np.meshgrid(np.arange(n), np.arange(hw[0]), np.arange(hw[1]), indexing='ij')
    idx = (nn * out_full_hw[0] + oy * out_stride) * out_full_hw[1] + ox * out_stride + out_pixel_offset
    assert idx.min() >= 0 and idx.max() < n * out_full_hw[0] * out_full_hw[1], 'the scatter leaves the output tensor'
    assert np.unique(idx).size == idx.size
    return idx


def gathered(full, hw, out_stride, out_pixel_offset):
    """what a scattered launch reads of a full-size residual / mask (N, out_H, out_W, C): the shifted, strided positions"""
    n, oh, ow, c = full.shape
    return full.reshape(-1, c)[scatter_pixels(n, hw, (oh, ow), out_stride, out_pixel_offset)]


def scattered(values, into, out_stride, out_pixel_offset):
    """`values` (N, Ho, Wo, C) placed into a copy of the pre-filled `into` (N, out_H, out_W, C) -> (array, visited (N, out_H, out_W)):
    positions the launch must not touch keep `into`'s value."""
    n, oh, ow, c = into.shape
    idx = scatter_pixels(n, values.shape[1:3], (oh, ow), out_stride, out_pixel_offset)
    out = np.array(into, dtype=values.dtype).reshape(-1, c)
    out[idx.ravel()] = values.reshape(-1, c)
    visited = np.zeros(n * oh * ow, dtype=bool)
    visited[idx.ravel()] = True
    return out.reshape(into.shape), visited.reshape(n, oh, ow)


def dgrad(du, wT, neg_taps, res=None, mask=None, out_hw=None):
    """mode 1 of the kernel: (conv(du, wT, neg_taps) + res) * [mask > 0], wT (taps, Cin, Cout) = the transposed, scale-folded weights
    -> (ref, A); A is gated like ref (a gated element is an exact zero)."""
    ref, A = epilogue(conv(du, wT, neg_taps, 1, out_hw), conv(np.abs(_f64(du)), np.abs(_f64(wT)), neg_taps, 1, out_hw), res=res)
    if mask is not None:
        gate = _f64(mask) > 0.0
        ref, A = np.where(gate, ref, 0.0), np.where(gate, A, 0.0)
    return ref, A


def _wgrad_sum(du, x, taps, stride):
    n, ho, wo, cout = du.shape
    h, wd, cin = x.shape[1:]
    dw = np.zeros((len(taps), cout, cin))
    for t in range(len(taps)):
        ys, xs, iy, ix = _tap_window(t, taps, stride, (h, wd), (ho, wo))
        if ys.size == 0 or xs.size == 0:
            continue
        g = du[np.ix_(np.arange(n), ys, xs)].reshape(-1, cout)
        dw[t] = g.T @ x[:, iy][:, :, ix].reshape(-1, cin)
    return dw


def wgrad(du, x, taps, stride=1, scale=None, cout_real=None, dw_cout=None, prefill=0.0):
    """dw[t, co, ci] = prefill + scale[co] * sum_pixels du[pix, co] * x[pix through tap t, ci] for co < cout_real; rows cout_real ..
    dw_cout - 1 stay at `prefill` -> (ref, A) of shape (taps, dw_cout, Cin); A = |prefill| + |scale| sum |du| |x|, 0 on the rows that
    are not written."""
    du, x = _f64(du), _f64(x)
    cout = du.shape[3]
    cout_real = cout if cout_real is None else cout_real
    dw_cout = cout if dw_cout is None else dw_cout
    assert cout_real <= dw_cout and cout_real <= cout
    s = np.ones(cout) if scale is None else _f64(scale)
    part = _wgrad_sum(du, x, taps, stride) * s[None, :, None]
    Apart = _wgrad_sum(np.abs(du), np.abs(x), taps, stride) * np.abs(s)[None, :, None]
    ref = np.full((len(taps), dw_cout, x.shape[3]), float(prefill))
    A = np.zeros_like(ref)
    ref[:, :cout_real] += part[:, :cout_real]
    A[:, :cout_real] = abs(float(prefill)) + Apart[:, :cout_real]
    return ref, A


def pack_transpose(w, scale=None, flip=False):
    """out[t', ci, co] = w[t, co, ci] * scale[co] in np.float32 (ONE fp32 product per element: bit-exact), t' = taps - 1 - t when
    `flip`."""
    w = np.asarray(w, dtype=np.float32)
    if scale is not None:
        w = w * np.asarray(scale, dtype=np.float32)[None, :, None]
    out = np.ascontiguousarray(w.transpose(0, 2, 1))
    return out[::-1].copy() if flip else out          # (.copy(): a one-tap array reversed keeps its negative stride otherwise)


def phase_taps(taps, py, px):
    """stride-2 data gradient as the phases of a transposed convolution: the input pixel (2 a + py, 2 b + px) receives through forward
    tap (dy, dx) from the output pixel (a + (py - dy) / 2, b + (px - dx) / 2), so the phase uses the taps with py - dy and px - dx even
    -> [(index of the forward tap, (row offset, column offset) into the output-gradient map)]"""
    return [(t, ((py - dy) // 2, (px - dx) // 2)) for t, (dy, dx) in enumerate(taps) if (py - dy) % 2 == 0 and (px - dx) % 2 == 0]


# ------------------------------------------------------------------------------------------------------------ launches
PIXEL_TILE = 128             # pixels per workgroup of conv_f32_kernel, every instance
K_STAGE = 32                 # input channels per stage
WGRAD_STAGE = 32             # pixels per stage of conv_wgrad_f32_kernel
WGRAD_TARGET = 384           # workgroups the automatic split aims at

FwdPlan = collections.namedtuple('FwdPlan', 'tile channel_tiles m pixel_tiles tail stages_per_tap ksplit taps_per_split split_taps')
WgradPlan = collections.namedtuple('WgradPlan', 'bco bci tiles ksplit per last_slice last_stage')


def fwd_plan(cin, cout, m, ntaps, ksplit=1):
    """cms_conv_igemm_f32: the channel tile is the largest of 128 / 64 / 32 that divides Cout; 128 pixels per workgroup (tail = the
    pixels of a last partial tile, 0 = none); Cin / 32 stages per tap; split s takes taps [s * tps, min(taps, (s + 1) * tps)), tps =
    ceil(taps / ksplit) -- `split_taps` lists their counts, a 0 is an empty split."""
    assert cin % K_STAGE == 0 and cout % 32 == 0 and 1 <= max(1, ksplit) <= ntaps
    tile = 128 if cout % 128 == 0 else 64 if cout % 64 == 0 else 32
    ks = max(1, ksplit)
    tps = -(-ntaps // ks)
    split_taps = tuple(max(0, min(ntaps, (s + 1) * tps) - s * tps) for s in range(ks))
    assert sum(split_taps) == ntaps
    return FwdPlan(tile, cout // tile, m, -(-m // PIXEL_TILE), m % PIXEL_TILE, cin // K_STAGE, ks, tps, split_taps)


def forward_bound(A, plan, cin, operands):
    """d = taps in the split x Cin + the splits (when there are several) + one per epilogue operand (module docstring)"""
    return bound(A, plan.taps_per_split * cin + (plan.ksplit if plan.ksplit > 1 else 0) + operands)


def wgrad_plan(cin, cout, m, ntaps, ksplit=0):
    """cms_conv_wgrad_f32: 128-wide tiles on an axis that is a multiple of 128, else 64; ksplit 0 = ceil(384 / tiles); the slice
    length is ceil(M / ksplit) rounded up to whole 32-pixel stages, and the number of slices follows from it (a request above M / 32
    is clamped that way). `last_stage` = pixels of the final partial stage of the last slice (0 = it is full)."""
    assert cin % 64 == 0 and cout % 64 == 0
    bco, bci = (128 if cout % 128 == 0 else 64), (128 if cin % 128 == 0 else 64)
    tiles = (cout // bco) * (cin // bci) * ntaps
    k = ksplit if ksplit > 0 else -(-WGRAD_TARGET // tiles)
    per = max(WGRAD_STAGE, -(-(-(-m // k)) // WGRAD_STAGE) * WGRAD_STAGE)
    k = -(-m // per)
    last = m - (k - 1) * per
    return WgradPlan(bco, bci, tiles, k, per, last, last % WGRAD_STAGE)


def wgrad_bound(A, plan):
    """d = pixels per slice + slices; A already holds |prefill| (`wgrad`)"""
    return bound(A, plan.per + plan.ksplit)


# ------------------------------------------------------------------------------------------------------------ cases
# `convs` = ((k, dilation, padding), ...): the taps of several convolutions of one input side by side (the ASPP head: 2 x 9 taps)
FCase = collections.namedtuple('FCase', 'name n h w cin cout convs stride cout_real tile pixel_tiles tail stages why seed')
WCase = collections.namedtuple('WCase', 'name n h w cin cout convs stride cout_real dw_cout tile why seed')
HEAD_KSPLITS = (1, 4, 5, 7, 18)
WGRAD_KSPLITS = (0, 1, 3, 1000)
PREFILL = 0.25               # content of the weight-gradient buffer before the launch
FILL = -3.5                  # content of a caller-owned scatter output before the launch

FORWARD = [
    FCase('k1_m35', 1, 5, 7, 32, 32, ((1, 1, 0),), 1, None, 32, 1, 35, 1, 'one K stage, one partial pixel tile, 32-tile', 201),
    FCase('cin96_t32', 2, 9, 15, 96, 96, ((3, 1, 1),), 1, None, 32, 3, 14, 3, 'odd stage count per tap, three 32-tiles, pixel tail', 202),
    FCase('t64_exact', 1, 16, 16, 64, 192, ((3, 2, 2),), 1, None, 64, 2, 0, 2, '64-tile, no tail', 203),
    FCase('t64_m129', 1, 3, 43, 32, 64, ((1, 1, 0),), 1, None, 64, 2, 1, 1, '64-tile, tail of one row', 204),
    FCase('t128_s2', 2, 11, 13, 64, 128, ((3, 1, 1),), 2, None, 128, 1, 84, 2, '128-tile, strided input walk, M < 128', 205),
    FCase('head18', 2, 9, 11, 64, 32, ((3, 6, 6), (3, 12, 12)), 1, 21, 32, 2, 70, 2, 'ksplit 1, 4, 5, 7, 18; NCHW output, bias', 206),
]
F = {c.name: c for c in FORWARD}
EPILOGUE_CASES = [F['cin96_t32'], F['t64_exact']]
EPILOGUES = collections.OrderedDict([            # mode 0: (scale, bias, res, relu)
    ('plain', (0, 0, 0, 0)), ('scale', (1, 0, 0, 0)), ('bias', (0, 1, 0, 0)), ('scale_bias', (1, 1, 0, 0)), ('relu', (0, 0, 0, 1)),
    ('res', (0, 0, 1, 0)), ('res_relu', (0, 0, 1, 1)), ('scale_bias_res_relu', (1, 1, 1, 1))])
GATES = collections.OrderedDict([('neither', (0, 0)), ('mask', (1, 0)), ('res', (0, 1)), ('mask_res', (1, 1))])      # mode 1: (mask, res)

WGRAD = [
    WCase('w64x64_m35', 1, 5, 7, 64, 64, ((1, 1, 0),), 1, None, None, (64, 64), '<1,1>, one full stage + 3 pixels', 301),
    WCase('w128x64', 2, 9, 15, 64, 128, ((3, 2, 2),), 1, None, None, (128, 64), '<2,1>', 302),
    WCase('w64x128_s2', 2, 11, 13, 128, 64, ((3, 1, 1),), 2, None, None, (64, 128), '<1,2>, strided', 303),
    WCase('w128x128_m9', 1, 3, 3, 128, 128, ((1, 1, 0),), 1, None, None, (128, 128), '<2,2>, M < 32', 304),
    WCase('whead18', 2, 9, 11, 64, 64, ((3, 6, 6), (3, 12, 12)), 1, 21, 32, (64, 64), 'padded classes, 18 taps', 305),
]
PACK_SHAPES = [(1, 32, 32), (9, 21, 40), (18, 33, 65)]           # (taps, Cout, Cin)


def case_taps(case):
    return [t for k, dil, pad in case.convs for t in conv_taps(k, dil, pad)]


def case_out_hw(case):
    k, dil, pad = case.convs[0]
    hw = conv_out(case.h, k, dil, pad, case.stride), conv_out(case.w, k, dil, pad, case.stride)
    assert all((conv_out(case.h, *c, case.stride), conv_out(case.w, *c, case.stride)) == hw for c in case.convs)
    return hw


def case_m(case):
    ho, wo = case_out_hw(case)
    return case.n * ho * wo


_f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
FInputs = collections.namedtuple('FInputs', 'x w scale bias res mask')
WInputs = collections.namedtuple('WInputs', 'du x scale')
SInputs = collections.namedtuple('SInputs', 'du wT res mask')


def _mask(rng, shape):
    """a ReLU output's sign pattern as the gate sees it: about half positive, and exact +0.0 / -0.0 (gated: the test is `> 0`)"""
    m = rng.randn(*shape)
    z = rng.rand(*shape)
    m[z < 0.125] = 0.0
    m[z < 0.0625] = -0.0
    return m


def forward_inputs(case):
    """fp32 operands of a forward case (numpy): x, w ~ N(0, 1) (w scaled to O(1) outputs), scale in [0.5, 1.5), bias ~ 0.2 N(0, 1), and
    a residual and a mask of the output's shape. In mode 1 the same x, w, taps are the gradient, the transposed weights and the
    negated taps of a data-gradient launch."""
    rng = np.random.RandomState(case.seed)
    ho, wo = case_out_hw(case)
    ntaps = len(case_taps(case))
    x = rng.randn(case.n, case.h, case.w, case.cin)
    w = rng.randn(ntaps, case.cout, case.cin) * (2.0 / case.cin) ** 0.5
    scale, bias = rng.rand(case.cout) + 0.5, rng.randn(case.cout) * 0.2
    res = rng.randn(case.n, ho, wo, case.cout)
    return FInputs(_f32(x), _f32(w), _f32(scale), _f32(bias), _f32(res), _f32(_mask(rng, res.shape)))


def wgrad_inputs(case):
    """du (N, Ho, Wo, Cout) -- random in the padded channels too, so a row beyond cout_real that is written shows --, x, scale"""
    rng = np.random.RandomState(case.seed)
    ho, wo = case_out_hw(case)
    return WInputs(_f32(rng.randn(case.n, ho, wo, case.cout)), _f32(rng.randn(case.n, case.h, case.w, case.cin)),
                   _f32(rng.rand(case.cout) + 0.5))


SCATTER = F['t128_s2']
PHASES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def scatter_inputs():
    """the t128_s2 operands as a data gradient: du of the forward OUTPUT's shape (2, 6, 7, 128), wT = the re-packed (scale folded)
    weights (9, 64, 128), residual and mask of the forward INPUT's shape (2, 11, 13, 64)"""
    c = SCATTER
    i = forward_inputs(c)
    rng = np.random.RandomState(c.seed + 1000)
    ho, wo = case_out_hw(c)
    du = rng.randn(c.n, ho, wo, c.cout)
    res = rng.randn(c.n, c.h, c.w, c.cin)
    return SInputs(_f32(du), pack_transpose(i.w, i.scale, False), _f32(res), _f32(_mask(rng, res.shape)))


def scatter_phase(py, px):
    """-> (tap indices into wT, (dy, dx) of the launch, (Ho, Wo) of the launch, out_pixel_offset) of phase (py, px)"""
    c = SCATTER
    sel = phase_taps(case_taps(c), py, px)
    return [t for t, _ in sel], [o for _, o in sel], ((c.h - py + 1) // 2, (c.w - px + 1) // 2), py * c.w + px


# ------------------------------------------------------------------------------------------------------------ mutations
# what a subtly wrong kernel would have to produce, built from the reference; tests/test_conv_f32_refs_cpu.py asserts that each lies
# OUTSIDE the bound the GPU test uses, at every case it applies to
def probe_tap(case):
    """the tap a K-stage mutation drops: (0, 0), which no pixel sees outside the map"""
    return case_taps(case).index((0, 0))


def asymmetric_tap(case):
    """first tap with dy != dx, or None (1 x 1 kernels)"""
    return next((t for t, (dy, dx) in enumerate(case_taps(case)) if dy != dx), None)


def drop_k_stage(acc, x, w, taps, stride, out_hw, tap, pixel_tile):
    """(a) the bare sum `acc` without the LAST 32-channel K stage of `tap`, in the pixels of ONE 128-pixel tile only"""
    part = conv(_f64(x)[..., -K_STAGE:], _f64(w)[tap:tap + 1, :, -K_STAGE:], [taps[tap]], stride, out_hw)
    out = acc.copy().reshape(-1, acc.shape[3])
    sl = slice(PIXEL_TILE * pixel_tile, PIXEL_TILE * (pixel_tile + 1))
    out[sl] -= part.reshape(out.shape)[sl]
    return out.reshape(acc.shape)


def bias_every_split(ref, bias, ksplit):
    """(b) every split adds the bias (the empty ones too) instead of split 0 alone"""
    return ref + (ksplit - 1) * _f64(bias)


def res_after_gate(du, wT, neg_taps, res, mask, out_hw=None):
    """(c) acc * [mask > 0] + res instead of (acc + res) * [mask > 0]"""
    return np.where(_f64(mask) > 0.0, conv(du, wT, neg_taps, 1, out_hw), 0.0) + _f64(res)


def drop_last_stage(du, plan, which_slice):
    """(d) du with the pixels of the final PARTIAL 32-pixel stage of slice `which_slice` zeroed -> (du, pixels dropped): what the
    weight gradient sums when that stage is skipped"""
    m = du.shape[0] * du.shape[1] * du.shape[2]
    begin, end = which_slice * plan.per, min(m, (which_slice + 1) * plan.per)
    n = (end - begin) % WGRAD_STAGE
    out = np.array(du, dtype=np.float64).reshape(m, -1)
    out[end - n:end] = 0.0
    return out.reshape(du.shape), n


def swap_tap_at_row(acc, x, w, taps, stride, out_hw, tap, row):
    """(e) output row `row` of every image computed with (dy, dx) of `tap` swapped"""
    swapped = list(taps)
    swapped[tap] = (taps[tap][1], taps[tap][0])
    out = acc.copy()
    out[:, row] = conv(x, w, swapped, stride, out_hw)[:, row]
    return out
