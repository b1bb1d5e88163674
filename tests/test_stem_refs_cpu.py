"""
CPU: the references of tests/_stem_refs.py against torch in fp64 (F.conv2d and autograd) at every geometry
tests/test_gpu_stem_kernels.py uses (the persistent case at a batch of 4 of the same distribution: the reference has no batch-dependent
code), and the SENSITIVITY of the bounds those GPU tests assert: a weight gradient that lacks one tile of the persistent case, or a
forward tile computed from the previous tile's patch, must lie outside the bound. This is what makes the references trustworthy, and
the bounds meaningful, without a GPU.

Agreement is to fp64 rounding: 1e-12 relative to A (the sum of absolute values of the same expression) on every element -- the sums
have at most 147 x 80 850 terms, torch and numpy order them differently, and 2^-53 x sqrt(terms) stays below 1e-12.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stem_refs as S
from _stream_refs import worst_ratio

REL = 1e-12
_id = lambda c: c.name


def _close(a, b, A, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    assert (err <= REL * A).all(), (what, float((err - REL * A).max()))


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _w_oihw(w):                  # (49, 64, 3) -> torch's (64, 3, 7, 7)
    return _t(w).reshape(7, 7, 64, 3).permute(2, 3, 0, 1).contiguous()


def _pack49(w):                  # and back
    return w.permute(2, 3, 0, 1).reshape(49, 64, 3).numpy()


@pytest.mark.parametrize('case', S.CASES, ids=_id)
def test_references_vs_conv2d_and_autograd_fp64(case):
    i = S.case_inputs(case, n=min(case.n, 4))
    x, w = _t(i.x).requires_grad_(True), _w_oihw(i.w).requires_grad_(True)
    sc, bi = _t(i.scale).view(1, -1, 1, 1), _t(i.bias).view(1, -1, 1, 1)
    conv = F.conv2d(x, w, None, 2, 3)
    assert S.stem_out_hw(case.h, case.w) == tuple(conv.shape[2:])
    ref, A = S.stem_forward(i.x, i.w, i.scale, i.bias)
    _close(ref, F.relu(conv * sc + bi).detach().permute(0, 2, 3, 1).numpy(), A, 'forward')
    Aw = F.conv2d(x.detach().abs(), w.detach().abs(), None, 2, 3) * sc.abs() + bi.abs()
    _close(A, Aw.permute(0, 2, 3, 1).numpy(), A, 'forward A')
    assert (A >= np.abs(ref) * (1 - 1e-12)).all()
    # backward of sum(conv * scale * dS): the gradients the two backward kernels compute
    g = _t(i.ds).permute(0, 3, 1, 2)
    (conv * sc * g).sum().backward()
    dw, Adw = S.stem_wgrad(i.x, i.ds, i.scale)
    _close(dw, _pack49(w.grad), Adw, 'wgrad')
    dx, Adx, taps = S.stem_dgrad(i.ds, i.w, i.scale, (case.h, case.w))
    _close(dx, x.grad.numpy(), Adx, 'dgrad')
    # A of both: the same graph on absolute values
    xa, wa = x.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
    (F.conv2d(xa, wa, None, 2, 3) * sc.abs() * g.abs()).sum().backward()
    _close(Adw, _pack49(wa.grad), Adw, 'wgrad A')
    _close(Adx, xa.grad.numpy(), Adx, 'dgrad A')
    # scale None is scale one
    dw1, Adw1 = S.stem_wgrad(i.x, i.ds, None)
    dwo, Adwo = S.stem_wgrad(i.x, i.ds, np.ones(64))
    assert np.array_equal(dw1, dwo) and np.array_equal(Adw1, Adwo)
    # taps: the number of kernel positions that reach an output pixel = the gradient of a convolution of ones with ones
    one = torch.ones(1, 1, case.h, case.w, dtype=torch.float64, requires_grad=True)
    F.conv2d(one, torch.ones(1, 1, 7, 7, dtype=torch.float64), None, 2, 3).sum().backward()
    assert np.array_equal(taps, np.rint(one.grad[0, 0].numpy()).astype(np.int64))
    assert taps.min() >= 1 and taps.max() <= 16


@pytest.mark.parametrize('hw', [(1, 1), (2, 7), (5, 40), (6, 6), (7, 8), (8, 6), (9, 9), (16, 34), (33, 47), (49, 97), (321, 321)])
def test_stem_out_hw_is_torchs(hw):
    y = F.conv2d(torch.zeros(1, 3, *hw), torch.zeros(64, 3, 7, 7), None, 2, 3)
    assert S.stem_out_hw(*hw) == tuple(y.shape[2:])


def test_bf16_round_is_torchs_and_the_weights_are_not_bf16():
    a = np.random.RandomState(0).randn(4096).astype(np.float32)
    a[:4] = [0.0, 1.0, 1.00390625, 1.01171875]                     # exact, exact, and the two ties of the even rule
    assert np.array_equal(S.bf16_round(a), torch.from_numpy(a).bfloat16().float().numpy())
    for case in S.CASES:
        w = S.case_inputs(case, n=1).w
        assert (S.bf16_round(w) != w).mean() > 0.95


def test_case_geometry_reaches_what_it_is_there_for():
    """the persistent case gives every persistent loop a second trip (and the matrix-core weight gradient a third); the reduce cases
    have one tile per image in both tilings; 16x34 has a one-pixel ragged tile column"""
    c = S.PERSISTENT
    assert S.stem_out_hw(c.h, c.w) == (25, 49)
    assert S.n_tiles(c.n, c.h, c.w, S.FWD_TILE) == 528 > S.FWD_CAP
    pm, pv = S.wgrad_plan(True, True, c.n, c.h, c.w), S.wgrad_plan(False, False, c.n, c.h, c.w)
    assert (pm.ntiles, pm.nblocks, pv.ntiles, pv.nblocks) == (528, 256, 1056, 768) and pm.ntiles > 2 * pm.nblocks
    assert S.wgrad_depth(pm) == 3 * 256 + 256 and S.wgrad_depth(pv) == 2 * 128 + 768
    for r in S.REDUCE:
        for bf in (False, True):
            p = S.wgrad_plan(bf, bf, r.n, r.h, r.w)
            assert p.ntiles == p.nblocks == r.n
    assert sorted(r.n for r in S.REDUCE) == [1, 3, 5, 13, 17]
    assert S.stem_out_hw(16, 34) == (8, 17)
    small = [S.stem_out_hw(e.h, e.w) for e in S.EDGES if e.h < 7 or e.w < 7]
    assert (1, 1) in small and all(min(s) <= 3 for s in small)


# ---------------------------------------------------------------------------------------------------------- sensitivity
@functools.lru_cache(maxsize=None)
def _persistent(x_bf16, ds_bf16):
    i = S.case_inputs(S.PERSISTENT)
    x, ds = S.typed(i.x, x_bf16), S.typed(i.ds, ds_bf16)
    return i, x, ds


# the four type pairs of the GPU test x scale given / None: each has its own bound (tile size, block cap, A)
@pytest.mark.parametrize('with_scale', [True, False], ids=['scale', 'noscale'])
@pytest.mark.parametrize('pair', [(False, False), (True, True), (False, True), (True, False)], ids=['f32xf32', 'bf16xbf16', 'f32xbf16', 'bf16xf32'])
def test_weight_gradient_bound_notices_one_dropped_tile(pair, with_scale):
    """CONDITION, not a measurement: on the persistent case, with the bound the GPU test asserts (wgrad_bound: pre-filled buffer, d
    from wgrad_depth), the reference without ONE tile is outside the bound on at least one element -- for tile 0, the last tile
    (the ragged corner: 9 x 1 pixels in the 16 x 16 tiling, ONE pixel in the 8 x 16 tiling), the first tile of a second trip (tile
    index = block count) and the last full-height tile of the one-pixel column. The fp32 pair has the loosest bound (8 x 16 tiles,
    768 blocks: d = 1024 for a 128-pixel tile); the 'positive' distribution of the case is what makes it hold."""
    i, x, ds = _persistent(*pair)
    scale = i.scale if with_scale else None
    plan = S.wgrad_plan(pair[0], pair[1], S.PERSISTENT.n, S.PERSISTENT.h, S.PERSISTENT.w)
    ref, A = S.stem_wgrad(x, ds, scale)
    bnd = S.wgrad_bound(A, S.PREFILL, plan)
    assert worst_ratio(ref + S.PREFILL, ref + S.PREFILL, bnd) == 0.0
    corner_column = plan.tiles_x - 1                                  # image 0, first tile row, the 1-pixel-wide column
    for t, pixels in ((0, plan.pixels), (plan.ntiles - 1, 9 if plan.mfma else 1), (plan.nblocks, plan.pixels),
                      (corner_column, plan.tile[0])):
        bad, dropped = S.drop_tile(x, ds, scale, ref, t, plan)
        assert dropped == pixels, (t, dropped)
        r = worst_ratio(bad + S.PREFILL, ref + S.PREFILL, bnd)
        print('SENSITIVITY wgrad {} tile {} ({} px): {:.2f} x the bound'.format(plan, t, dropped, r))
        assert r > 1.0, (t, r)


@pytest.mark.parametrize('bf16_out', [True, False], ids=['bf16out', 'fp32out'])
def test_forward_bound_notices_a_stale_patch(bf16_out):
    """a forward whose tile was computed from the patch of the tile the same workgroup took one trip earlier (t - 512: the missing
    loop-head barrier of stem_fwd_mfma_kernel) is outside the matrix-core bound, for the first and the last second-trip tile"""
    i, x, _ = _persistent(True, True)
    ref, A = S.stem_forward(x, i.w, i.scale, i.bias)
    bnd = S.forward_bound(A, ref, bf16_out, mfma=True)
    nt = S.n_tiles(S.PERSISTENT.n, S.PERSISTENT.h, S.PERSISTENT.w, S.FWD_TILE)
    for t in (S.FWD_CAP, nt - 1):
        bad = S.stale_tile_forward(x, i.w, i.scale, i.bias, ref, t, t - S.FWD_CAP)
        r = worst_ratio(bad, ref, bnd)
        print('SENSITIVITY forward tile {} from the patch of {}: {:.1f} x the bound'.format(t, t - S.FWD_CAP, r))
        assert r > 1.0, (t, r)
    # ... and the helper is the reference when the patch is the tile's own
    for t in (0, 7, nt - 1):
        _close(S.stale_tile_forward(x, i.w, i.scale, i.bias, ref, t, t), ref, A, 'own patch')
