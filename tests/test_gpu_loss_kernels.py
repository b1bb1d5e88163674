"""
GPU tests of csrc/losses.hip on the tile paths the older geometries do not reach (`-m gpu`): the comparing loop of the x-adjoint
(more than 24 low-resolution columns per tile, or more than 20 tile columns per low-resolution column), the launches above 48 KB of
LDS, the direct-gather forward kernels of non-identity geometries and the "too many classes at this scale" error. Every geometry
runs through the three ways a gradient is produced -- the one-launch `*_fused`, the forward + backward pair, and the pair under
cms_loss_set_deterministic(1) -- and EACH is held to the fp64 reference of tests/_loss_refs.py (pinned on the CPU by
tests/test_loss_refs_cpu.py, which also asserts the path of every geometry here):

  exact cases     dyadic bilinear weights, integer logits, C = 4, logits_var, power-of-two factors: every intermediate is an fp32
                  number, the gradient must EQUAL the reference whatever the order of the atomics (torch.equal)
  bounded cases   |got - ref| <= (d + 2) u32 U^T|f g| + U^T(|f| K u32 a_k (1 + L)) on every element, K = 4 x the measured kappa
                  (_loss_refs; + (d + 2) 2^-126 for results below fp32's normal range); the scalars to the same construction over the pixel sum; rate and valid count exactly

Each test prints `RATIO <case> <worst |got - ref| / bound>` (`-s` shows them).
"""
import ctypes

import numpy as np
import pytest
import torch

import _loss_refs as L
import _stream_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROUTES = ('fused', 'pair', 'pair_det')
U32 = L.U32


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


def cu(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _Deterministic(object):
    """cms_loss_set_deterministic(on) for the block, the session's setting restored behind it"""

    def __init__(self, ops, on):
        from cutmix_semisup_seg_amd._lib import fn
        self.fn, self.ops, self.on = fn, ops, on

    def __enter__(self):
        self.fn['cms_loss_set_deterministic'](1 if self.on else 0)

    def __exit__(self, *exc):
        self.fn['cms_loss_set_deterministic'](1 if self.ops.deterministic_wgrad() else 0)


def run_consistency(ops, route, geo, combo, i, ramp=L.RAMP, weight=L.WEIGHT, invert=True, grad_init=None, samples=None, facts=True):
    """-> (scalars fp64 [4], gradient fp32 numpy) of one route"""
    from cutmix_semisup_seg_amd._lib import fn as cfn
    N, C, h, w, H, W, ac = geo
    fn, mode, tau, pp = combo
    cfg = ops.ConsistencyConfig(mode=mode, loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=ac, invert=invert)
    args = (cfg, cu(i['ls']), cu(i['l0']), cu(i['l1']) if mode == 'mix' else None, (H, W))
    rg = i.get('ranges')
    kw = dict(ranges=None if rg is None else ops.ranges_to_device(rg, DEV), mask=cu(i.get('mask')), um0=cu(i['um0']),
              um1=cu(i['um1']) if mode == 'mix' else None, ramp_val=ramp, cons_weight=weight)
    g = torch.zeros(N, C, h, w, device=DEV) if grad_init is None else cu(grad_init).clone()
    with _Deterministic(ops, route == 'pair_det'):
        if route == 'fused':
            assert grad_init is None and samples is None
            if facts:
                rd = ops._nonempty_ranges(kw['ranges'])           # (what the wrappers hand to the library for zero boxes)
                d = ops._cons_desc(cfg, args[1], args[2], args[3], rd, kw['mask'], kw['um0'], kw['um1'], (H, W))
                assert cfn['cms_consistency_fused_supported'](ctypes.byref(d)) == int(L.tile_facts(C, h, w, H, W, ac, 3)['fused'])
            sc = ops.consistency_fused(*args, g, **kw)
        else:
            sc, ctx = ops.consistency_forward(*args, **kw)
            ops.consistency_backward(ctx, sc, g, samples=samples)
        torch.cuda.synchronize()
    return sc.cpu().numpy().astype(np.float64), g.cpu().numpy()


def check_scalars(sc, ref, weight, what):
    closs, rate, gscale, unsup = ref['scalars']
    b = ref['sbound']
    for got, want, bnd, tag in ((sc[0], closs, b, 'closs'), (sc[3], unsup, b * abs(weight) + U32 * abs(unsup), 'unsup')):
        print('RATIO {} {} {:.4f}'.format(what, tag, R.worst_ratio(got, want, bnd)))
        assert np.isfinite(got) and abs(got - want) <= bnd, (what, tag, got, want, bnd)
    if np.isnan(rate):
        assert np.isnan(sc[1]), (what, sc[1])
    else:
        assert sc[1] == float(np.float32(rate)), (what, sc[1], rate)          # a count over P: exact
    assert abs(sc[2] - gscale) <= 2 * U32 * abs(gscale), (what, sc[2], gscale)


def check_consistency(sc, g, ref, what, weight=L.WEIGHT):
    check_scalars(sc, ref, weight, what)
    return R.assert_within(g, ref['grad'], ref['bound'], what + ' grad')


# ------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('mode', ['mix', 'cut'])
@pytest.mark.parametrize('name', list(L.EXACT_GEOS))
def test_exact_gradient_on_dyadic_geometries(ops, name, mode, route):
    """nothing rounds (tests/test_loss_refs_cpu.py::test_exact_cases_are_representable_in_fp32): a dropped, doubled or mis-weighted
    contribution of the staging, the x-adjoint (comparing loop in `cmp33`, table in the other two, a partial second tile in
    `tab2part`) or the y-adjoint cannot hide behind a tolerance"""
    geo = L.EXACT_GEOS[name]
    N, C, h, w, H, W, ac = geo
    i = L.exact_inputs(name, mode)
    ref = L.consistency(i['ls'], i['l0'], i['l1'], H, W, ac, mode, 'logits_var', 0.0, False, ranges=i.get('ranges'), mask=i.get('mask'),
                        um0=i['um0'], um1=i['um1'], ramp=i['ramp'], weight=i['weight'])
    sc, g = run_consistency(ops, route, geo, ('logits_var', mode, 0.0, False), i, ramp=i['ramp'], weight=i['weight'])
    want = ref['grad'].astype(np.float32)
    assert np.abs(want).max() > 0
    assert torch.equal(torch.from_numpy(g), torch.from_numpy(want)), (name, mode, route, int((g != want).sum()), float(np.abs(g - want).max()))
    check_scalars(sc, L.slim(ref), i['weight'], 'exact {} {} {}'.format(name, mode, route))


# ------------------------------------------------------------------------------------------------------------ bounded cases
_CASES = [(n, c) for n in L.GEOS if L.GEOS[n][9]['backward'] != 'error' for c in L.combos_of(n)]     # (not 'toobig', 'ce46')


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name,combo', _CASES, ids=['{}-{}-{}-{}'.format(n, c[0], c[1], int(c[3])) for n, c in _CASES])
def test_consistency_within_the_bound(ops, name, combo, route):
    geo = L.GEOS[name][:7]
    sc, g = run_consistency(ops, route, geo, combo, L.case_inputs(name, combo[1]))
    check_consistency(sc, g, L.reference(name, combo), 'cons {} {} {} {}'.format(name, combo[0], combo[1], route))


def run_ce(ops, route, geo, lo, y, weight=1.0):
    from cutmix_semisup_seg_amd._lib import fn as cfn
    N, C, h, w, H, W, ac = geo
    lo_d, y_d = cu(lo), cu(y)
    g = torch.zeros(N, C, h, w, device=DEV)
    with _Deterministic(ops, route == 'pair_det'):
        if route == 'fused':
            d = ops._ce_desc(lo_d, y_d, 255, (H, W), ac)
            assert cfn['cms_ce_fused_supported'](ctypes.byref(d)) == int(L.tile_facts(C, h, w, H, W, ac, 1)['fused'])
            sc = ops.ce_fused(lo_d, y_d, g, (H, W), 255, ac, loss_weight=weight)
        else:
            sc, ctx = ops.ce_forward(lo_d, y_d, (H, W), 255, ac, loss_weight=weight)
            ops.ce_backward(ctx, sc, g)
        torch.cuda.synchronize()
    return sc.cpu().numpy().astype(np.float64), g.cpu().numpy()


def check_ce(sc, g, ref, what):
    val, gscale = ref['scalars']
    print('RATIO {} value {:.4f}'.format(what, R.worst_ratio(sc[0], val, ref['sbound'])))
    assert np.isfinite(sc[0]) and abs(sc[0] - val) <= ref['sbound'], (what, sc[0], val, ref['sbound'])
    assert sc[1] == float(np.float32(gscale)), (what, sc[1], gscale, ref['n_valid'])      # weight / n_valid: the count is exact
    return R.assert_within(g, ref['grad'], ref['bound'], what + ' grad')


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name', list(L.GEOS))
def test_cross_entropy_within_the_bound(ops, name, route):
    lo, y = L.ce_inputs(name)
    sc, g = run_ce(ops, route, L.GEOS[name][:7], lo, y)
    check_ce(sc, g, L.ce_reference(name), 'ce {} {}'.format(name, route))


# ------------------------------------------------------------------------------------------------------------ no tiled launch
def test_too_many_classes_at_this_scale_is_an_error_and_touches_nothing(ops):
    """32 classes at 60 x 60 -> 65 x 65 need 182 KB of LDS for the tiled consistency backward: no fused launch, the forward runs on
    the direct-gather kernel, the backward returns the library's error through `check` -- no launch, `grad_out` as it was"""
    from cutmix_semisup_seg_amd._lib import fn as cfn, CmsError
    name = 'toobig'
    geo = L.GEOS[name][:7]
    N, C, h, w, H, W, ac = geo
    assert L.tile_facts(C, h, w, H, W, ac, 3)['backward'] == 'error'
    for combo in L.combos_of(name):
        fn, mode, tau, pp = combo
        i = L.case_inputs(name, mode)
        ref = L.reference(name, combo)
        cfg = ops.ConsistencyConfig(mode=mode, loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=ac)
        args = (cfg, cu(i['ls']), cu(i['l0']), cu(i['l1']) if mode == 'mix' else None, (H, W))
        kw = dict(ranges=ops.ranges_to_device(i['ranges'], DEV), um0=cu(i['um0']), um1=cu(i['um1']) if mode == 'mix' else None,
                  ramp_val=L.RAMP, cons_weight=L.WEIGHT)
        d = ops._cons_desc(cfg, args[1], args[2], args[3], kw['ranges'], None, kw['um0'], kw['um1'], (H, W))
        for det in (False, True):
            with _Deterministic(ops, det):
                assert cfn['cms_consistency_fused_supported'](ctypes.byref(d)) == 0
                sc, ctx = ops.consistency_forward(*args, **kw)
                torch.cuda.synchronize()
                check_scalars(sc.cpu().numpy().astype(np.float64), ref, L.WEIGHT, 'toobig fwd {} det{}'.format(fn, int(det)))
                g = torch.full((N, C, h, w), 1.5, device=DEV)
                with pytest.raises((ValueError, CmsError), match='32 classes at this scale need 181632 B of LDS'):
                    ops.consistency_backward(ctx, sc, g)
                g2 = torch.full((N, C, h, w), 1.5, device=DEV)
                with pytest.raises((ValueError, CmsError), match='need 181632 B of LDS'):
                    ops.consistency_fused(*args, g2, **kw)
                torch.cuda.synchronize()
                assert torch.equal(g, torch.full_like(g, 1.5)) and torch.equal(g2, torch.full_like(g2, 1.5))
    # (the cross entropy of the same shape stages one tensor, 104 KB: test_cross_entropy_within_the_bound[toobig-*])


# ------------------------------------------------------------------------------------------------------------ further cases
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name', ['pm60_kld', 'pm60_bce', 'pm60_bce4'])
def test_logits_of_60_where_exponentials_underflow(ops, name, route):
    """t == 0 in KLD, 1 - p + eps == eps in BCE: finite and within the bound"""
    geo, combo, build = L.EXTRA[name]
    sc, g = run_consistency(ops, route, geo, combo, build())
    assert np.isfinite(sc[[0, 2, 3]]).all() and np.isfinite(g).all()
    check_consistency(sc, g, L.extra_reference(name), '{} {}'.format(name, route))


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('name', L.AT_TAU)
def test_confidence_exactly_at_the_threshold_counts(ops, name, route):
    """uniform teacher logits: conf == 1 / C == tau in every pixel; `>=` keeps them all (rate 1) and they carry gradient"""
    geo, combo, build = L.EXTRA[name]
    sc, g = run_consistency(ops, route, geo, combo, build())
    ref = L.extra_reference(name)
    assert sc[1] == 1.0 and ref['scalars'][1] == 1.0
    assert np.abs(g).max() > 0.1 * np.abs(ref['grad']).max() > 0
    check_consistency(sc, g, ref, '{} {}'.format(name, route))


@pytest.mark.parametrize('invert', [True, False])
@pytest.mark.parametrize('nb', [0, 1, 3])
def test_box_ranges_and_the_equivalent_float_mask(ops, nb, invert):
    """0, 1 and 3 overlapping boxes, rasterised in-kernel or given as a float mask (0.75 / 0.25): the same result -- to the bit where
    the order of the sums is fixed (scalars; gradient of the colour-class launches) -- and each within the bound of the reference"""
    name = 'boxes%d' % nb
    geo, combo, build = L.EXTRA[name]
    N, C, h, w, H, W, ac = geo
    i = build()
    assert i['ranges'].shape == (N, nb, 4)
    ref = L.extra_reference(name, invert)
    im = dict(i)
    im['ranges'] = None
    im['mask'] = L.box_mask(i['ranges'], H, W, invert).astype(np.float32)[:, None] * 0.5 + 0.25
    for route in ROUTES:
        sc_r, g_r = run_consistency(ops, route, geo, combo, i, invert=invert)
        sc_m, g_m = run_consistency(ops, route, geo, combo, im, invert=invert)
        what = '{} inv{} {}'.format(name, int(invert), route)
        check_consistency(sc_r, g_r, ref, what + ' ranges')
        check_consistency(sc_m, g_m, ref, what + ' mask')
        assert np.array_equal(sc_r, sc_m, equal_nan=True), (what, sc_r, sc_m)
        if route == 'pair_det':
            assert np.array_equal(g_r, g_m), what


@pytest.mark.parametrize('route', ROUTES)
def test_validity_weights_zero_and_fractional(ops, route):
    geo, combo, build = L.EXTRA['um_zero']
    sc, g = run_consistency(ops, route, geo, combo, build())
    assert sc[0] == 0.0 and sc[3] == 0.0 and not g.any()
    geo, combo, build = L.EXTRA['um_0.3']
    sc, g = run_consistency(ops, route, geo, combo, build())
    check_consistency(sc, g, L.extra_reference('um_0.3'), 'um_0.3 {}'.format(route))


def _tiles_touching(in_size, out_size, ac, tile):
    i0, i1, _, _ = R.bilinear_taps(in_size, out_size, ac, np.float32)
    t = np.arange(out_size) // tile
    return np.array([len(set(t[(i0 == c) | (i1 == c)])) for c in range(in_size)])


@pytest.mark.parametrize('det', [False, True])
def test_pair_accumulates_into_grad_out_and_over_a_run_of_samples(ops, det):
    """the backward ADDS to a non-zero `grad_out` (one atomic add per tile that touches a cell: n_t further roundings at the size of
    the running value), and samples=(1, 3) writes rows 1:3 only -- on a geometry of the comparing loop (33 columns)"""
    geo, combo, build = L.EXTRA['three']
    N, C, h, w, H, W, ac = geo
    assert N == 3 and not L.tile_facts(C, h, w, H, W, ac, 3)['table_all']
    i = build()
    ref = L.extra_reference('three')
    init = (np.random.RandomState(5).randn(N, C, h, w) * 1e-3).astype(np.float32)
    n_t = np.outer(_tiles_touching(h, H, ac, L.TILE_H), _tiles_touching(w, W, ac, L.TILE_W))[None, None]
    route = 'pair_det' if det else 'pair'
    want = init.astype(np.float64) + ref['grad']
    bnd = ref['bound'] + n_t * U32 * (np.abs(init) + np.abs(want) + ref['bound'])
    sc, g = run_consistency(ops, route, geo, combo, i, grad_init=init)
    check_scalars(sc, ref, L.WEIGHT, 'three ' + route)
    R.assert_within(g, want, bnd, 'three accumulate ' + route)
    sc, g = run_consistency(ops, route, geo, combo, i, grad_init=init, samples=(1, 3))
    assert np.array_equal(g[0], init[0])
    R.assert_within(g[1:], want[1:], np.broadcast_to(bnd, want.shape)[1:], 'three samples(1,3) ' + route)
    sc, g0 = run_consistency(ops, route, geo, combo, i, samples=(0, 1))
    assert not g0[1:].any()
    R.assert_within(g0[:1], ref['grad'][:1], ref['bound'][:1], 'three samples(0,1) ' + route)


@pytest.mark.parametrize('route', ROUTES)
def test_cross_entropy_int64_labels_outside_the_classes(ops, route):
    """negative labels, labels >= C and labels beyond 2^31 are skipped like the ignore value: count, value and gradient"""
    lo, y = L.ce_i64_inputs()
    N, C, h, w, H, W, ac = L.G_TP
    ref = L.slim(L.cross_entropy(lo, y, H, W, ac))
    assert ref['n_valid'] < 0.7 * y.size
    sc, g = run_ce(ops, route, L.G_TP, lo, y, weight=0.5)
    ref['scalars'] = (ref['scalars'][0], 0.5 * ref['scalars'][1])
    ref['grad'], ref['bound'] = 0.5 * ref['grad'], 0.5 * ref['bound']
    check_ce(sc, g, ref, 'ce int64 ' + route)
