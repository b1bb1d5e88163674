"""
CPU: the references of tests/_conv_f32_refs.py against torch in fp64 (F.conv2d and autograd) at every case
tests/test_gpu_conv_f32_kernels.py uses -- the NCHW / cout_real, scattered and dw_cout forms included --, the GEOMETRY of every case
against the launchers' rules (tile, pixel tiles and tail, stages per tap, taps per split and empty splits, slice length and last
partial stage), and the SENSITIVITY of the bounds the GPU test asserts: five mutations of the reference -- a dropped K stage in one
pixel tile, the bias added by every split, the residual added behind the mask gate, a dropped partial stage of the weight gradient, one
tap transposed at a border row -- must each lie outside the bound at every case they apply to.

Agreement is to fp64 rounding: 1e-12 relative to A (the sum of absolute values of the same expression) on every element.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_f32_refs as C
from _stream_refs import worst_ratio

REL = 1e-12
_id = lambda c: c.name


def _close(a, b, A, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    assert (err <= REL * A).all(), (what, float((err - REL * A).max()))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _oihw(w9):                   # (k * k, Cout, Cin) -> torch's (Cout, Cin, k, k)
    k = int(round(w9.shape[0] ** 0.5))
    return w9.reshape(k, k, w9.shape[1], w9.shape[2]).permute(2, 3, 0, 1).contiguous()


def _packed(w):                  # and back
    co, ci, k, _ = w.shape
    return w.permute(2, 3, 0, 1).reshape(k * k, co, ci)


def _torch_conv(case, x_nchw, ws):
    """the case's convolutions (one, or the head's two side by side) of one input, summed; `ws` = one OIHW weight per convolution"""
    return sum(F.conv2d(x_nchw, w, None, case.stride, pad, dil) for w, (k, dil, pad) in zip(ws, case.convs))


def _split_weights(case, w):
    """(taps, Cout, Cin) -> one OIHW leaf per convolution of the case"""
    out, t0 = [], 0
    for k, _, _ in case.convs:
        out.append(_oihw(_t(w)[t0:t0 + k * k]).requires_grad_(True))
        t0 += k * k
    return out


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


@functools.lru_cache(maxsize=None)
def _finputs(case):
    return C.forward_inputs(case)


@functools.lru_cache(maxsize=None)
def _winputs(case):
    return C.wgrad_inputs(case)


# ====================================================================================================== references vs torch
@pytest.mark.parametrize('case', C.FORWARD, ids=_id)
def test_forward_and_data_gradient_vs_conv2d_and_autograd_fp64(case):
    i = _finputs(case)
    taps, (ho, wo) = C.case_taps(case), C.case_out_hw(case)
    x = _t(i.x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ws = _split_weights(case, i.w)
    sc, bi = _t(i.scale).view(1, -1, 1, 1), _t(i.bias).view(1, -1, 1, 1)
    res = _t(i.res).permute(0, 3, 1, 2)
    y = _torch_conv(case, x, ws)
    assert tuple(y.shape[2:]) == (ho, wo)
    Ay = _torch_conv(case, x.detach().abs(), [w.detach().abs() for w in ws])
    for name, (s, b, r, relu) in C.EPILOGUES.items():
        ref, A = C.forward(i.x, i.w, taps, case.stride, (ho, wo), i.scale if s else None, i.bias if b else None, i.res if r else None,
                           bool(relu))
        want, Aw = y.detach(), Ay
        if s:
            want, Aw = want * sc, Aw * sc.abs()
        if b:
            want, Aw = want + bi, Aw + bi.abs()
        if r:
            want, Aw = want + res, Aw + res.abs()
        if relu:
            want = F.relu(want)
        _close(ref, _nhwc(want), A, 'forward ' + name)
        _close(A, _nhwc(Aw), A, 'forward A ' + name)
        assert (A >= np.abs(ref) * (1 - 1e-12)).all()
        # the NCHW form with cout_real is the same numbers, transposed and cut
        cr = case.cout_real or case.cout
        n_ref = C.nchw(ref, cr)
        assert n_ref.shape == (case.n, cr, ho, wo) and n_ref.flags['C_CONTIGUOUS']
        _close(n_ref, want.numpy()[:, :cr], C.nchw(A, cr), 'forward NCHW ' + name)
    # data gradient of sum(conv(x, w) * scale * dU) = conv of dU with the transposed, scale-folded weights and the negated taps
    rng = np.random.RandomState(case.seed + 50)
    du = rng.randn(case.n, ho, wo, case.cout)
    (y * sc * _t(du).permute(0, 3, 1, 2)).sum().backward()
    wT = C.pack_transpose(i.w, None, False).astype(np.float64) * i.scale.astype(np.float64)[None, None, :]
    neg = [(-dy, -dx) for dy, dx in taps]
    add, mask = rng.randn(case.n, case.h, case.w, case.cin), C._mask(rng, (case.n, case.h, case.w, case.cin))
    xa = x.detach().abs().requires_grad_(True)
    (_torch_conv(case, xa, [w.detach().abs() for w in ws]) * sc.abs() * _t(np.abs(du)).permute(0, 3, 1, 2)).sum().backward()
    if case.stride == 1:
        for gname, (m, r) in C.GATES.items():
            ref, A = C.dgrad(du, wT, neg, add if r else None, mask if m else None, (case.h, case.w))
            want, Aw = _nhwc(x.grad), _nhwc(xa.grad)
            if r:
                want, Aw = want + add, Aw + np.abs(add)
            if m:
                want, Aw = want * (mask > 0), Aw * (mask > 0)
            _close(ref, want, Aw, 'dgrad ' + gname)
            _close(A, Aw, Aw, 'dgrad A ' + gname)
            if m:
                assert (ref[mask <= 0] == 0).all() and (A[mask <= 0] == 0).all()
    else:
        # the four phases of the transposed convolution, each scattered into the full map, add up to the gradient
        total, seen = np.zeros((case.n, case.h, case.w, case.cin)), np.zeros((case.n, case.h, case.w), dtype=int)
        for py, px in C.PHASES:
            sel = C.phase_taps(taps, py, px)
            hw = ((case.h - py + 1) // 2, (case.w - px + 1) // 2)
            ref, _ = C.dgrad(du, wT[[t for t, _ in sel]], [o for _, o in sel], None, None, hw)
            out, visited = C.scattered(ref, np.zeros_like(total), 2, py * case.w + px)
            total, seen = total + out, seen + visited
        assert (seen == 1).all()
        _close(total, _nhwc(x.grad), _nhwc(xa.grad), 'dgrad as four phases')


def test_scattered_form_places_gathers_and_leaves_the_rest():
    """the scattered reference the GPU test uses: per phase, residual and mask are read at the shifted positions, the result is placed
    there, every other position keeps the fill -- and the four phases (residual and mask from the full maps) are the gated gradient"""
    c, s = C.SCATTER, C.scatter_inputs()
    i = _finputs(c)
    assert s.du.shape == (2, 6, 7, 128) and s.wT.shape == (9, 64, 128) and s.res.shape == (2, 11, 13, 64)
    x = torch.zeros(c.n, c.cin, c.h, c.w, dtype=torch.float64, requires_grad=True)
    ws = _split_weights(c, i.w)
    (_torch_conv(c, x, ws) * _t(i.scale).view(1, -1, 1, 1) * _t(s.du).permute(0, 3, 1, 2)).sum().backward()
    # (wT folds the scale in fp32; the autograd graph above in fp64: compare through the fp64 product of the same fp32 numbers)
    wT64 = C.pack_transpose(i.w, None, False).astype(np.float64) * i.scale.astype(np.float64)[None, None, :]
    total, seen = np.zeros(s.res.shape), np.zeros(s.res.shape[:3], dtype=int)
    offsets = []
    for py, px in C.PHASES:
        idx, taps, hw, off = C.scatter_phase(py, px)
        offsets.append(off)
        assert len(idx) == {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4}[(py, px)]
        ref, A = C.dgrad(s.du, wT64[idx], taps, C.gathered(s.res, hw, 2, off), C.gathered(s.mask, hw, 2, off), hw)
        fill = np.full(s.res.shape, C.FILL)
        out, visited = C.scattered(ref, fill, 2, off)
        assert visited.sum() == c.n * hw[0] * hw[1] and (out[~visited] == C.FILL).all()
        assert np.array_equal(out[:, py::2, px::2], ref) and visited[:, py::2, px::2].all()
        total, seen = total + np.where(visited[..., None], out, 0.0), seen + visited
    assert offsets == [0, 1, c.w, c.w + 1] and (seen == 1).all()
    want = (_nhwc(x.grad) + s.res.astype(np.float64)) * (s.mask > 0)
    _close(total, want, np.abs(want) + 1.0, 'scattered phases')


@pytest.mark.parametrize('case', C.WGRAD, ids=_id)
def test_weight_gradient_vs_autograd_fp64(case):
    i = _winputs(case)
    taps = C.case_taps(case)
    x = _t(i.x).permute(0, 3, 1, 2).contiguous()
    ws = [torch.zeros(case.cout, case.cin, k, k, dtype=torch.float64, requires_grad=True) for k, _, _ in case.convs]
    g = _t(i.du).permute(0, 3, 1, 2)
    assert tuple(g.shape[2:]) == C.case_out_hw(case)
    for scale in (i.scale, None):
        for w in ws:
            w.grad = None
        sc = _t(i.scale if scale is not None else np.ones(case.cout)).view(1, -1, 1, 1)
        (_torch_conv(case, x, ws) * sc * g).sum().backward()
        want = np.concatenate([_packed(w.grad).numpy() for w in ws])
        wa = [torch.zeros_like(w).requires_grad_(True) for w in ws]
        (_torch_conv(case, x.abs(), wa) * sc.abs() * g.abs()).sum().backward()
        Aw = np.concatenate([_packed(w.grad).numpy() for w in wa])
        cr, dc = case.cout_real or case.cout, case.dw_cout or case.cout
        ref, A = C.wgrad(i.du, i.x, taps, case.stride, scale, case.cout_real, case.dw_cout, C.PREFILL)
        assert ref.shape == (len(taps), dc, case.cin)
        _close(ref[:, :cr], C.PREFILL + want[:, :cr], C.PREFILL + Aw[:, :cr], 'wgrad')
        _close(A[:, :cr], C.PREFILL + Aw[:, :cr], C.PREFILL + Aw[:, :cr], 'wgrad A')
        assert (ref[:, cr:] == C.PREFILL).all() and (A[:, cr:] == 0).all()          # rows that are not written: exact, bound 0
    one, _ = C.wgrad(i.du, i.x, taps, case.stride, np.ones(case.cout), case.cout_real, case.dw_cout, C.PREFILL)
    assert np.array_equal(one, ref)                                                 # scale None is scale one


@pytest.mark.parametrize('flip', [True, False])
@pytest.mark.parametrize('shape', C.PACK_SHAPES, ids=str)
def test_pack_transpose_is_torchs_fp32_product(shape, flip):
    rng = np.random.RandomState(sum(shape))
    w, scale = rng.randn(*shape).astype(np.float32), (rng.rand(shape[1]) + 0.5).astype(np.float32)
    for s in (scale, None):
        tw = torch.from_numpy(w)
        if s is not None:
            tw = tw * torch.from_numpy(s).view(1, -1, 1)
        want = tw.permute(0, 2, 1).flip(0) if flip else tw.permute(0, 2, 1)
        got = C.pack_transpose(w, s, flip)
        assert got.dtype == np.float32 and got.shape == (shape[0], shape[2], shape[1]) and got.flags['C_CONTIGUOUS']
        assert torch.equal(torch.from_numpy(got), want.contiguous())


# ====================================================================================================== geometry
def test_case_geometry_reaches_what_it_is_there_for():
    """every case, recomputed from the launchers' rules (C.fwd_plan / C.wgrad_plan restate cms_conv_igemm_f32 / cms_conv_wgrad_f32),
    lands on the tile, the pixel tiles and tail, the stages per tap, the split and the slice its name says"""
    for c in C.FORWARD:
        taps = C.case_taps(c)
        p = C.fwd_plan(c.cin, c.cout, C.case_m(c), len(taps))
        assert (p.tile, p.pixel_tiles, p.tail, p.stages_per_tap) == (c.tile, c.pixel_tiles, c.tail, c.stages), (c.name, p)
    f = C.F
    assert C.case_m(f['k1_m35']) == 35 and C.case_m(f['cin96_t32']) == 270 == 2 * 128 + 14 and C.case_m(f['t64_exact']) == 256
    assert C.case_m(f['t64_m129']) == 129 and C.case_out_hw(f['t128_s2']) == (6, 7) and C.case_m(f['t128_s2']) == 84 < 128
    assert C.fwd_plan(96, 96, 270, 9).channel_tiles == 3 and C.fwd_plan(64, 192, 256, 9).channel_tiles == 3
    assert f['cin96_t32'].stages % 2 == 1 and f['k1_m35'].stages == 1 and f['t64_m129'].tail == 1
    # every tile size, with and without a tail, one and several pixel tiles
    assert {c.tile for c in C.FORWARD} == {32, 64, 128}
    assert {(c.tile, c.tail > 0) for c in C.FORWARD} >= {(32, True), (64, True), (64, False), (128, True)}
    # the head: 18 taps, all but the centre of the 12-dilated nine outside a 9 x 11 map; the splits the issue lists
    h = f['head18']
    taps = C.case_taps(h)
    assert len(taps) == 18 and h.cout_real == 21 < h.cout == 32
    outside = [t for t, (dy, dx) in enumerate(taps) if abs(dy) >= h.h or abs(dx) >= h.w]
    assert outside == [9, 10, 11, 12, 14, 15, 16, 17]
    plans = {k: C.fwd_plan(h.cin, h.cout, C.case_m(h), 18, k) for k in C.HEAD_KSPLITS}
    assert plans[1].split_taps == (18,)
    assert plans[4].split_taps == (5, 5, 5, 3)                    # ragged last split
    assert plans[5].split_taps == (4, 4, 4, 4, 2)                 # ragged last split
    assert plans[7].split_taps == (3, 3, 3, 3, 3, 3, 0)           # the last split is empty
    assert plans[18].split_taps == (1,) * 18
    # the strided scatter: launches of 1, 2, 2, 4 taps on the 64-channel tile, offsets 0, 1, W, W + 1
    for (py, px), ntaps in zip(C.PHASES, (1, 2, 2, 4)):
        idx, taps, hw, off = C.scatter_phase(py, px)
        p = C.fwd_plan(C.SCATTER.cout, C.SCATTER.cin, C.SCATTER.n * hw[0] * hw[1], len(idx))
        assert len(idx) == ntaps and p.tile == 64 and p.stages_per_tap == 4 and off == py * 13 + px
    # weight gradient: the tile pair, and per requested split the slice length, the slices and the last partial stage
    want = {
        #                 ksplit 0 (automatic)      1                3               1000 (clamped to M / 32 slices)
        'w64x64_m35':  {0: (32, 2, 3),    1: (64, 1, 3),    3: (32, 2, 3),   1000: (32, 2, 3)},
        'w128x64':     {0: (32, 9, 14),   1: (288, 1, 14),  3: (96, 3, 14),  1000: (32, 9, 14)},
        'w64x128_s2':  {0: (32, 3, 20),   1: (96, 1, 20),   3: (32, 3, 20),  1000: (32, 3, 20)},
        'w128x128_m9': {0: (32, 1, 9),    1: (32, 1, 9),    3: (32, 1, 9),   1000: (32, 1, 9)},
        'whead18':     {0: (32, 7, 6),    1: (224, 1, 6),   3: (96, 3, 6),   1000: (32, 7, 6)},
    }
    for c in C.WGRAD:
        m, ntaps = C.case_m(c), len(C.case_taps(c))
        for k in C.WGRAD_KSPLITS:
            p = C.wgrad_plan(c.cin, c.cout, m, ntaps, k)
            assert (p.bco, p.bci) == c.tile and (p.per, p.ksplit, p.last_stage) == want[c.name][k], (c.name, k, p)
            assert p.per % 32 == 0 and (p.ksplit - 1) * p.per < m <= p.ksplit * p.per and p.last_stage == m % 32 != 0
    assert {c.tile for c in C.WGRAD} == {(64, 64), (128, 64), (64, 128), (128, 128)}
    assert C.case_m(C.WGRAD[0]) == 35 == 32 + 3 and C.case_m(C.WGRAD[3]) == 9 < 32
    w = C.WGRAD[4]
    assert (w.cout, w.cout_real, w.dw_cout, len(C.case_taps(w))) == (64, 21, 32, 18)
    # a slice with a partial stage that is NOT the only stage of its slice: 96 = 2 full stages + 14 in the last of three slices
    assert C.wgrad_plan(64, 128, 270, 9, 3).last_slice == 78 == 2 * 32 + 14


# ====================================================================================================== sensitivity
def _operands(s, b, r):
    return int(bool(s)) + int(bool(b)) + int(bool(r))


@pytest.mark.parametrize('case', C.FORWARD, ids=_id)
def test_forward_bound_notices_a_dropped_k_stage_in_one_pixel_tile(case):
    """(a) the last 32 input channels of ONE tap missing in ONE 128-pixel tile (the first and the last -- the tail -- in turn), under
    the plain and the full epilogue (the head: bias, every ksplit): outside the bound the GPU test asserts"""
    i = _finputs(case)
    taps, hw, m = C.case_taps(case), C.case_out_hw(case), C.case_m(case)
    acc = C.conv(i.x, i.w, taps, case.stride, hw)
    Aacc = C.conv(np.abs(i.x), np.abs(i.w), taps, case.stride, hw)
    if case.cout_real:
        epis = [((None, i.bias, None, False), k) for k in C.HEAD_KSPLITS]
    else:
        epis = [((None, None, None, False), 1), ((i.scale, i.bias, i.res, True), 1)]
    for (s, b, r, relu), ksplit in epis:
        plan = C.fwd_plan(case.cin, case.cout, m, len(taps), ksplit)
        ref, A = C.epilogue(acc, Aacc, s, b, r, relu)
        bnd = C.forward_bound(A, plan, case.cin, _operands(s is not None, b is not None, r is not None))
        for tile in sorted({0, plan.pixel_tiles - 1}):
            bad, _ = C.epilogue(C.drop_k_stage(acc, i.x, i.w, taps, case.stride, hw, C.probe_tap(case), tile), Aacc, s, b, r, relu)
            lo, hi = tile * 128, min(m, tile * 128 + 128)
            diff = (bad != ref).reshape(m, -1).any(axis=1)
            assert diff[lo:hi].any() and not diff[:lo].any() and not diff[hi:].any()
            ratio = worst_ratio(bad, ref, bnd)
            print('SENSITIVITY {} dropped K stage, tile {} ksplit {}: {:.0f} x the bound'.format(case.name, tile, ksplit, ratio))
            assert ratio > 1.0, (case.name, tile, ratio)


@pytest.mark.parametrize('ksplit', [k for k in C.HEAD_KSPLITS if k > 1])
def test_forward_bound_notices_the_bias_added_by_every_split(ksplit):
    """(b) on head18, every ksplit > 1 (7: the empty split adds it too)"""
    case = C.F['head18']
    i = _finputs(case)
    taps, hw = C.case_taps(case), C.case_out_hw(case)
    ref, A = C.forward(i.x, i.w, taps, 1, hw, None, i.bias)
    plan = C.fwd_plan(case.cin, case.cout, C.case_m(case), 18, ksplit)
    bnd = C.nchw(C.forward_bound(A, plan, case.cin, 1), case.cout_real)
    ratio = worst_ratio(C.nchw(C.bias_every_split(ref, i.bias, ksplit), case.cout_real), C.nchw(ref, case.cout_real), bnd)
    print('SENSITIVITY head18 bias in each of {} splits: {:.0f} x the bound'.format(ksplit, ratio))
    assert ratio > 1.0


@pytest.mark.parametrize('case', C.EPILOGUE_CASES + ['scatter'], ids=lambda c: getattr(c, 'name', c))
def test_data_gradient_bound_notices_the_residual_added_behind_the_gate(case):
    """(c) (acc + res) * gate vs acc * gate + res: differs exactly on the gated elements, where the bound is zero"""
    if case == 'scatter':
        s = C.scatter_inputs()
        idx, taps, hw, off = C.scatter_phase(1, 1)
        du, wT, res, mask = s.du, s.wT[idx], C.gathered(s.res, hw, 2, off), C.gathered(s.mask, hw, 2, off)
        cin, m = C.SCATTER.cout, C.SCATTER.n * hw[0] * hw[1]
    else:
        i = _finputs(case)
        du, wT, taps, res, mask, hw = i.x, i.w, C.case_taps(case), i.res, i.mask, C.case_out_hw(case)
        cin, m = case.cin, C.case_m(case)
    ref, A = C.dgrad(du, wT, taps, res, mask, hw)
    bnd = C.forward_bound(A, C.fwd_plan(cin, wT.shape[1], m, len(taps)), cin, 1)
    bad = C.res_after_gate(du, wT, taps, res, mask, hw)
    assert ((bad != ref) == ((mask <= 0) & (res != 0))).all() and (mask == 0).any()
    assert worst_ratio(ref, ref, bnd) == 0.0 and worst_ratio(bad, ref, bnd) == np.inf


@pytest.mark.parametrize('with_scale', [True, False], ids=['scale', 'noscale'])
@pytest.mark.parametrize('ksplit', C.WGRAD_KSPLITS)
@pytest.mark.parametrize('case', C.WGRAD, ids=_id)
def test_weight_gradient_bound_notices_a_dropped_partial_stage(case, ksplit, with_scale):
    """(d) every case has M % 32 != 0, so the last slice of every split ends in a partial stage (3, 14, 20, 9, 6 pixels): the weight
    gradient without those pixels is outside the bound of that launch"""
    i = _winputs(case)
    taps = C.case_taps(case)
    plan = C.wgrad_plan(case.cin, case.cout, C.case_m(case), len(taps), ksplit)
    scale = i.scale if with_scale else None
    ref, A = C.wgrad(i.du, i.x, taps, case.stride, scale, case.cout_real, case.dw_cout, C.PREFILL)
    bnd = C.wgrad_bound(A, plan)
    du, dropped = C.drop_last_stage(i.du, plan, plan.ksplit - 1)
    assert dropped == plan.last_stage > 0
    bad, _ = C.wgrad(du, i.x, taps, case.stride, scale, case.cout_real, case.dw_cout, C.PREFILL)
    ratio = worst_ratio(bad, ref, bnd)
    print('SENSITIVITY {} ksplit {} without the last {} pixels: {:.0f} x the bound'.format(case.name, ksplit, dropped, ratio))
    assert worst_ratio(ref, ref, bnd) == 0.0 and ratio > 1.0


@pytest.mark.parametrize('case', [c for c in C.FORWARD if C.asymmetric_tap(c) is not None], ids=_id)
def test_forward_bound_notices_a_transposed_tap_at_a_border_row(case):
    """(e) the first tap with dy != dx read as (dx, dy) in output row 0 (where the true tap looks above the map) and in the last row"""
    i = _finputs(case)
    taps, hw, m = C.case_taps(case), C.case_out_hw(case), C.case_m(case)
    tap = C.asymmetric_tap(case)
    acc = C.conv(i.x, i.w, taps, case.stride, hw)
    Aacc = C.conv(np.abs(i.x), np.abs(i.w), taps, case.stride, hw)
    bias = i.bias if case.cout_real else None
    ref, A = C.epilogue(acc, Aacc, None, bias)
    for ksplit in (C.HEAD_KSPLITS if case.cout_real else (1,)):
        bnd = C.forward_bound(A, C.fwd_plan(case.cin, case.cout, m, len(taps), ksplit), case.cin, int(bias is not None))
        for row in (0, hw[0] - 1):
            bad, _ = C.epilogue(C.swap_tap_at_row(acc, i.x, i.w, taps, case.stride, hw, tap, row), Aacc, None, bias)
            assert np.array_equal(np.delete(bad, row, axis=1), np.delete(ref, row, axis=1))
            ratio = worst_ratio(bad, ref, bnd)
            print('SENSITIVITY {} tap {} transposed in row {} ksplit {}: {:.0f} x the bound'.format(case.name, taps[tap], row, ksplit, ratio))
            assert ratio > 1.0, (case.name, row, ratio)
