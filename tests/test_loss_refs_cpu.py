"""
CPU pins of tests/_loss_refs.py (no GPU): the fp64 restatement of the two losses reproduces the committed fixtures
(tests/golden/losses.npz) and agrees with oracle/losses.py run in fp64; `tile_facts` puts every geometry of
tests/test_gpu_loss_kernels.py on the kernel path it is there for (a drifting shape list fails HERE, not silently); the conditions
on the inputs hold (exact cases representable in fp32, no undecided confidence pixel); KAPPA is at least what the reference's own
formulas lose in fp32 on these inputs.
"""
import numpy as np
import pytest
import torch

import _loss_refs as L
from conftest import load_golden, load_golden_json

_LC = load_golden_json('losses_meta')


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize('case', _LC, ids=[c['key'] for c in _LC])
def test_reference_reproduces_the_committed_consistency_fixtures(case):
    """identity geometry (9 x 11), float mask: values and gradient at the tolerances tests/test_oracle_golden.py holds the oracle to"""
    g = load_golden('losses')
    pre = 'C{}__'.format(case['C'])
    a = lambda n: g[pre + n]
    H, W = a('l_stu').shape[2:]
    r = L.consistency(a('l_stu'), a('l0_tea'), a('l1_tea') if case['mode'] == 'mix' else None, H, W, True, case['mode'], case['fn'],
                      case['conf_thresh'], case['conf_per_pixel'], mask=a('mask'), um0=a('um0'),
                      um1=a('um1') if case['mode'] == 'mix' else None, ramp=case['ramp_val'] if case['rampup'] > 0 else 1.0,
                      weight=case['cons_weight'])
    closs, unsup, rate = g[case['key'] + '__vals']
    assert r['scalars'][0] == pytest.approx(closs, rel=2e-6, abs=1e-9)
    assert r['scalars'][3] == pytest.approx(unsup, rel=2e-6, abs=1e-9)
    if case['conf_thresh'] > 0:
        assert r['scalars'][1] == pytest.approx(rate, abs=1e-7)
    # the fixture's gradient is torch's fp32 autograd: it is held to this fp64 value within the reference's own fp32 bound
    want = g[case['key'] + '__grad'].astype(np.float64)
    assert (np.abs(r['grad'] - want) <= L.grad_bound(r) + 1e-5 * np.abs(want) + 1e-9).all()
    np.testing.assert_allclose(r['grad'], want, rtol=1e-3, atol=2e-5 * max(1e-12, np.abs(want).max()))


@pytest.mark.parametrize('C', [21, 2])
def test_reference_reproduces_the_committed_ce_fixtures(C):
    g = load_golden('losses')
    pre = 'C{}__'.format(C)
    lo = g[pre + 'l_stu']
    for dt in (np.uint8, np.int64):
        r = L.cross_entropy(lo, g[pre + 'labels'].astype(dt), lo.shape[2], lo.shape[3], True)
        assert r['scalars'][0] == pytest.approx(float(g[pre + 'ce__val']), rel=2e-6)
        np.testing.assert_allclose(r['grad'], g[pre + 'ce__grad'], rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------ oracle in fp64
def _t(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float64))


def _oracle_up(x, H, W, ac):
    # the SAME dense fp32-weight matrices (pinned against F.interpolate by tests/test_stream_refs_cpu.py), applied by torch so that
    # autograd runs through them: the comparison below is then about the losses, to fp64 rounding
    My, Mx, _ = L.matrices(x.shape[2], x.shape[3], H, W, ac)
    return torch.einsum('Yy,ncyx,Xx->ncYX', torch.tensor(My), x, torch.tensor(Mx))


_ORACLE_CASES = [(n, c) for n in L.GEOS for c in L.combos_of(n)]


@pytest.mark.parametrize('name,combo', _ORACLE_CASES, ids=['{}-{}-{}'.format(n, c[0], c[1]) for n, c in _ORACLE_CASES])
def test_reference_agrees_with_the_oracle_in_fp64(name, combo):
    from oracle import losses as olosses
    fn, mode, tau, pp = combo
    N, C, h, w, H, W, ac = L.GEOS[name][:7]
    i = L.case_inputs(name, mode)
    ref = L.reference(name, combo)
    ls = _t(i['ls']).requires_grad_(True)
    m = _t(L.box_mask(i['ranges'], H, W, True).astype(np.float64))[:, None]
    kw = dict(loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, ramp_val=L.RAMP, rampup=1, cons_weight=L.WEIGHT)
    up = lambda x: _oracle_up(x, H, W, ac)
    if mode == 'mix':
        r = olosses.mix_mode_loss(up(ls), up(_t(i['l0'])), up(_t(i['l1'])), m, _t(i['um0']), _t(i['um1']), **kw)
    else:
        r = olosses.cut_mode_loss(up(ls), up(_t(i['l0'])), m, _t(i['um0']), **kw)
    r['unsup_loss'].backward()
    assert ref['scalars'][0] == pytest.approx(float(r['consistency_loss'].detach()), rel=1e-11, abs=1e-15)
    assert ref['scalars'][3] == pytest.approx(float(r['unsup_loss'].detach()), rel=1e-11, abs=1e-15)
    if tau > 0:
        assert ref['scalars'][1] == pytest.approx(float(r['conf_rate']), abs=1e-15)
    want = ls.grad.numpy()
    np.testing.assert_allclose(ref['grad'], want, rtol=1e-9, atol=1e-13 * max(1e-30, np.abs(want).max()))


@pytest.mark.parametrize('name', list(L.GEOS))
def test_ce_reference_agrees_with_the_oracle_in_fp64(name):
    from oracle import losses as olosses
    N, C, h, w, H, W, ac = L.GEOS[name][:7]
    lo, y = L.ce_inputs(name)
    ref = L.ce_reference(name)
    lt = _t(lo).requires_grad_(True)
    ce = olosses.supervised_ce(_oracle_up(lt, H, W, ac), torch.tensor(y.astype(np.int64)))
    ce.backward()
    assert ref['scalars'][0] == pytest.approx(float(ce.detach()), rel=1e-11)
    want = lt.grad.numpy()
    np.testing.assert_allclose(ref['grad'], want, rtol=1e-9, atol=1e-13 * np.abs(want).max())


def test_ce_reference_skips_labels_outside_the_classes():
    """negative labels and labels >= C count as ignored (what the kernels do); torch's loss on the remaining labels is the value"""
    lo, y = L.ce_i64_inputs()
    N, C, h, w, H, W, ac = L.G_TP
    r = L.cross_entropy(lo, y, H, W, ac)
    y2 = np.where((y < 0) | (y >= C), 255, y)
    assert (y2 != y).sum() > 100 and r['n_valid'] == float((y2 != 255).sum())
    lt = _t(lo).requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(_oracle_up(lt, H, W, ac), torch.tensor(y2), ignore_index=255)
    ce.backward()
    assert r['scalars'][0] == pytest.approx(float(ce.detach()), rel=1e-11)
    np.testing.assert_allclose(r['grad'], lt.grad.numpy(), rtol=1e-9, atol=1e-15)


def test_box_mask_and_float_mask_are_the_same_paste():
    rng = np.random.RandomState(0)
    for nb in (0, 1, 3):
        ranges = L.boxes(rng, 2, 20, 30, nb)
        for inv in (True, False):
            bits = L.box_mask(ranges, 20, 30, inv)
            assert (L.paste_bits(2, 20, 30, mask=bits.astype(np.float32)[:, None] * 0.5 + 0.25) == bits).all()    # 0.75 / 0.25
            if nb == 0:
                assert (bits == (not inv)).all()
    from oracle import boxmask
    ranges = L.boxes(rng, 3, 33, 47, 3)
    for inv in (True, False):
        assert (boxmask.rasterise(ranges, (33, 47), inv).reshape(3, 33, 47).astype(bool) == L.box_mask(ranges, 33, 47, inv)).all()


# ------------------------------------------------------------------------------------------------------------ paths
@pytest.mark.parametrize('name', list(L.GEOS))
def test_every_geometry_is_on_the_path_it_is_there_for(name):
    N, C, h, w, H, W, ac = L.GEOS[name][:7]
    want = dict(L.GEOS[name][9])
    f = L.tile_facts(C, h, w, H, W, ac, 3)
    loop = want.pop('loop')
    assert f['table_all'] == (loop == 'table'), f
    want.setdefault('fused', True)
    for k, v in want.items():
        assert f[k] == v, (name, k, f)


def test_the_paths_of_the_issue_table():
    """the figures the geometries were chosen for"""
    F = lambda name, n_patches: L.tile_facts(*L.GEOS[name][1:7], n_patches)
    assert F('cmp33', 3)['r_n_cols'] == 33 > L.WT_COLS and F('sy1', 3)['r_n_cols'] == 34 and F('ratio2', 3)['r_n_cols'] == 34
    assert F('span38', 3)['span'] == 38 > L.WT_SPAN and F('span64', 3)['span'] == 64 and F('span42', 3)['span'] == 42
    assert F('span64', 3)['r_n_cols'] == 3 and F('span42', 3)['r_n_cols'] == 3
    assert F('one', 3)['r_n_cols'] == 1 and F('one', 3)['r_n_rows'] == 1 and F('onerow', 3)['r_n_rows'] == 1
    assert all(L.GEOS[n][4] % L.TILE_H != 0 and F(n, 3)['tiles_x'] == 2 for n in ('one', 'onerow'))
    assert F('tab2part', 3)['tiles_x'] == 2 and L.GEOS['tab2part'][5] % L.TILE_W == 32
    assert L.LDS_OPT_IN < F('ratio2', 3)['lds'] == 67536 and F('c40', 3)['lds'] == 62400 and F('c60', 3)['lds'] == 93600
    assert F('ratio2s', 3)['lds'] == 67536 and 24 < F('ratio2s', 3)['r_n_cols'] <= 32      # (25..32 columns: beside the table limit)
    n3, n1 = F('near1', 3), F('near1', 1)
    assert n3['fwd_lds'] == 138348 > L.FWD_PATCH_LDS_MAX and n3['forward'] == 'direct' and n3['lds'] == 119196 and n3['fused']
    assert n1['forward'] == 'tiled' and n1['lds'] == 67956 and n1['backward'] == 'tiled_optin'
    t3, t1 = F('toobig', 3), F('toobig', 1)
    assert t3['lds'] == 181632 > L.LDS_MAX and not t3['fused'] and t3['forward'] == 'direct' and t3['backward'] == 'error'
    assert t1['lds'] == 103552 and t1['fused'] and t1['backward'] == 'tiled_optin'
    c1 = F('ce46', 1)
    assert c1['fwd_lds'] == 46 * 9 * 62 * 4 > L.FWD_PATCH_LDS_MAX and c1['forward'] == 'direct' and c1['backward'] == 'tiled_optin' and c1['fused']
    assert F('identc3', 1)['forward'] == F('identc3', 1)['backward'] == 'identity' and not F('identc3', 1)['fused']
    # class counts: the compile-time 2, 5, 19, 21 and generic ones, C = 1 among them
    assert {2, 5, 19, 21, 1, 3, 4, 40, 60, 32} <= {g[1] for g in L.GEOS.values()}


def test_tile_facts_on_the_geometries_the_older_tests_use():
    """the corner the issue describes: every geometry of tests/test_gpu_parity.py sits on the table path below 48 KB"""
    for C, h, w, H, W, ac in [(5, 6, 7, 41, 50, True), (21, 41, 41, 321, 321, True), (19, 65, 129, 512, 1024, True),
                              (7, 9, 9, 33, 33, False), (21, 17, 17, 65, 65, False), (6, 9, 11, 40, 57, False), (5, 9, 9, 65, 65, True)]:
        f = L.tile_facts(C, h, w, H, W, ac, 3)
        assert f['table_all'] and f['r_n_cols'] <= 17 and f['span'] <= 17 and f['lds'] <= L.LDS_OPT_IN and f['forward'] == 'tiled', f


# ------------------------------------------------------------------------------------------------------------ inputs
def test_no_confidence_pixel_is_undecided():
    """zero exclusions: no pixel of any bounded case has |conf - tau| < 1e-5 (the two cases built to sit AT tau are exact there)"""
    for name in L.GEOS:
        for combo in L.combos_of(name):
            assert L.reference(name, combo)['conf_margin'] >= 1e-5, (name, combo)
    for name in L.EXTRA:
        for inv in ((True, False) if name.startswith('boxes') else (True,)):
            mg = L.extra_reference(name, inv)['conf_margin']
            assert (mg == 0.0) if name in L.AT_TAU else (mg >= 1e-5), (name, inv, mg)
    for name in L.AT_TAU:
        r = L.extra_reference(name, full=True)
        assert (r['conf'] == L.EXTRA[name][1][2]).all() and r['scalars'][1] == 1.0 and np.abs(r['grad']).max() > 0


@pytest.mark.parametrize('name', list(L.EXACT_GEOS))
@pytest.mark.parametrize('mode', ['mix', 'cut'])
def test_exact_cases_are_representable_in_fp32(name, mode):
    N, C, h, w, H, W, ac = L.EXACT_GEOS[name]
    i = L.exact_inputs(name, mode)
    r = L.consistency(i['ls'], i['l0'], i['l1'], H, W, ac, mode, 'logits_var', 0.0, False, ranges=i.get('ranges'), mask=i.get('mask'),
                      um0=i['um0'], um1=i['um1'], ramp=i['ramp'], weight=i['weight'])
    unit = i['ramp'] * i['weight'] / (N * H * W)
    assert np.log2(unit) == np.round(np.log2(unit)) and np.float32(i['weight']) == i['weight'] and np.float32(r['scalars'][2]) == r['scalars'][2]
    f32 = lambda a: (np.asarray(a).astype(np.float32).astype(np.float64) == a).all()
    assert f32(r['up_s']) and f32(r['up_t']) and f32(r['fg']) and f32(r['grad'])
    # ... and so is every partial sum, whatever the order: the sums of absolute values need no more than 24 bits
    A = L.adjoint(np.abs(r['fg']), h, w, ac)
    lsb = np.abs(r['fg'][r['fg'] != 0]).min() / 64.0          # weights are multiples of 2^-3 per axis: products of 2^-6
    assert A.max() / lsb < 2 ** 24 and np.abs(r['grad']).max() > 0
    bits = np.log2(A.max() / lsb)
    print('BITS {} {} {:.1f}'.format(name, mode, bits))


# ------------------------------------------------------------------------------------------------------------ kappa
def test_kappa_of_every_case_is_below_the_constant():
    """KAPPA / KAPPA_VALUE >= the largest |fp32 - fp64| / (u32 a (1 + L)) of the reference's own formulas on the tests' inputs"""
    worst, worst_v = {}, {}

    def note(fn, t32, t64):
        worst[fn] = max(worst.get(fn, 0.0), L.kappa(t32, t64))
        worst_v[fn] = max(worst_v.get(fn, 0.0), L.kappa(t32, t64, ('loss', 'aloss')))
    for name in L.GEOS:
        N, C, h, w, H, W, ac = L.GEOS[name][:7]
        for fn, mode, tau, pp in L.combos_of(name):
            i = L.case_inputs(name, mode)
            a = (i['ls'], i['l0'], i['l1'], H, W, ac, mode, fn, tau, pp)
            kw = dict(ranges=i['ranges'], um0=i['um0'], um1=i['um1'])
            note(fn, L.consistency(*a, dtype=np.float32, **kw)['terms'], L.consistency(*a, **kw)['terms'])
        lo, y = L.ce_inputs(name)
        note('ce', L.cross_entropy(lo, y, H, W, ac, dtype=np.float32)['terms'], L.cross_entropy(lo, y, H, W, ac)['terms'])
    for name, (geo, (fn, mode, tau, pp), build) in L.EXTRA.items():
        N, C, h, w, H, W, ac = geo
        i = build()
        a = (i['ls'], i['l0'], i['l1'] if mode == 'mix' else None, H, W, ac, mode, fn, tau, pp)
        kw = dict(ranges=i['ranges'], um0=i['um0'], um1=i['um1'] if mode == 'mix' else None)
        note(fn, L.consistency(*a, dtype=np.float32, **kw)['terms'], L.consistency(*a, **kw)['terms'])
    lo, y = L.ce_i64_inputs()
    note('ce', L.cross_entropy(lo, y, *L.G_TP[4:7], dtype=np.float32)['terms'], L.cross_entropy(lo, y, *L.G_TP[4:7])['terms'])
    print('KAPPA measured', {k: round(v, 3) for k, v in worst.items()}, 'values', {k: round(v, 3) for k, v in worst_v.items()})
    for fn in worst:
        assert worst[fn] <= L.KAPPA[fn] and worst_v[fn] <= L.KAPPA_VALUE[fn], (fn, worst[fn], worst_v[fn])
        assert worst[fn] > 0.25 * L.KAPPA[fn], (fn, worst[fn], 'the constant is not a measured one any more')
