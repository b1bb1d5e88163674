"""
GPU tests of the class-threshold consistency (csrc/cthresh.hip, `-m gpu`) against the fp64 restatement of tests/_cthresh_refs.py, whose
cases, threshold vectors, margins and bounds tests/test_cthresh_cpu.py pins on the CPU:

  kernels      every case x vector x route (forward + backward pair, the one fused launch where it exists): scalars and gradient within
               _loss_refs' bound construction, n_valid / N_pred / N_pass EQUAL, S_conf / S_c within the statistics bound
  equivalence  with thr == tau the scalars are bit for bit those of cms_consistency_*; the gradient is bit for bit theirs where the
               existing kernels reproduce themselves (the pair under cms_loss_set_deterministic(1), the identity backward). The
               default pair and the fused launch add tiles that share low-resolution cells with fp32 atomics in a run-dependent
               order -- two runs of cms_consistency_fwd_bwd do not give the same bits either -- so those routes are held to the bound.
  order        a batch in one call, in two calls and backward in samples= runs; repeated calls; a non-zero grad_out
  update       the launch against the restatement from the kernel's own integer table; three in a row; static mode
  refusal      `toobig`: the error code of cms_consistency_bwd, nothing touched, tables included
  the step     two iterations in freematch mode, the three routes, --deterministic, class_thresh=None
  trainer      --synthetic end to end, both modes
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import _cthresh_refs as R
import _loss_refs as L
import _stream_refs as S
import test_gpu_loss_kernels as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
cu = K.cu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


def thresholds(ops, thr):
    """a ClassThresholds whose vector is `thr` as it stands (zeros included, which a typed static list may not hold)"""
    ct = ops.ClassThresholds(len(thr), DEV, mode='freematch', ema=0.5, floor=0.0, ceil=1.0)
    ct.thr.copy_(torch.from_numpy(np.asarray(thr, dtype=np.float32)))
    return ct


def table(ct):
    return [int(v) for v in ct.iteration_table().cpu().numpy().astype(np.uint64)]


def run(ops, route, case, thr=None, tau=0.97, ct=None, grad_init=None, samples=None, rows=slice(None)):
    """one route of one case -> (scalars fp64[4], gradient numpy, ClassThresholds or None). `thr` None: the scalar threshold `tau`"""
    name, mode, fn, pp, given = case
    N, C, h, w, H, W, ac = R.geometry(name)
    i = R.inputs(case)
    if ct is None and thr is not None:
        ct = thresholds(ops, thr)
    cfg = ops.ConsistencyConfig(mode=mode, loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=ac, invert=True, class_thresh=ct)
    sl = lambda a: None if a is None else a[rows]
    args = (cfg, cu(sl(i['ls'])), cu(sl(i['l0'])), cu(sl(i['l1'])) if mode == 'mix' else None, (H, W))
    kw = dict(ranges=None if i['ranges'] is None else ops.ranges_to_device(sl(i['ranges']), DEV), mask=cu(sl(i['mask'])),
              um0=cu(sl(i['um0'])), um1=cu(sl(i['um1'])) if mode == 'mix' else None, ramp_val=R.RAMP, cons_weight=R.WEIGHT)
    g = torch.zeros(args[1].shape, device=DEV) if grad_init is None else cu(grad_init).clone()
    with K._Deterministic(ops, route == 'pair_det'):
        if route == 'fused':
            sc = ops.consistency_fused(*args, g, **kw)
        else:
            sc, ctx = ops.consistency_forward(*args, **kw)
            if samples is None:
                ops.consistency_backward(ctx, sc, g)
            else:
                for s in samples:
                    ops.consistency_backward(ctx, sc, g, samples=s)
        torch.cuda.synchronize()
    return sc.cpu().numpy().astype(np.float64), g.cpu().numpy(), ct


def check_table(got, ref, C, what):
    t, b = ref['table'], ref['table_bound']
    assert got[0] == t[0], (what, 'n_valid', got[0], t[0])
    assert got[2 + C:] == t[2 + C:], (what, 'N_pred / N_pass', got[2 + C:], t[2 + C:])
    for k in range(1, 2 + C):
        print('RATIO {} S[{}] {:.4f}'.format(what, k - 1, abs(got[k] - t[k]) / b[k] if b[k] else 0.0))
        assert abs(got[k] - t[k]) <= b[k], (what, k, got[k], t[k], b[k])


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('route', ['pair', 'fused'])
@pytest.mark.parametrize('vec', R.VECTORS)
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_kernels_against_the_restatement(ops, case, vec, route):
    name = case[0]
    C = R.geometry(name)[1]
    ref = R.reference(case, vec)
    assert ref['gap'] >= R.GAP and ref['conf_margin'] >= R.CONF              # the condition on the inputs, first
    if route == 'fused':
        # the fused launch exists exactly where cms_consistency_fused_supported says so (elsewhere ops runs the pair: the identity case)
        from cutmix_semisup_seg_amd._lib import fn as cfn, CthreshDesc
        ct = thresholds(ops, ref['thr'])
        N, _, h, w, H, W, ac = R.geometry(name)
        cfg = ops.ConsistencyConfig(mode=case[1], loss_fn=case[2], align_corners=ac, class_thresh=ct)
        z = torch.zeros(N, C, h, w, device=DEV)
        d = ops._cons_desc(cfg, z, z, z, None, torch.zeros(N, 1, H, W, device=DEV), None, None, (H, W))
        cd = ops._ct_desc(cfg, d)
        assert isinstance(cd, CthreshDesc)
        assert cfn['cms_cthresh_fused_supported'](ctypes.byref(cd)) == cfn['cms_consistency_fused_supported'](ctypes.byref(d)) \
            == int(R.ROUTES[name]['fused'])
    what = 'cthresh {} {} {}'.format(R.case_id(case), vec, route)
    sc, g, ct = run(ops, route, case, ref['thr'])
    K.check_consistency(sc, g, ref, what, weight=R.WEIGHT)
    check_table(table(ct), ref, C, what)


# ------------------------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize('route', ['pair', 'pair_det', 'fused'])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_constant_vector_equals_the_existing_kernels(ops, case, route):
    C = R.geometry(case[0])[1]
    for tau in (0.5, 0.9):
        a_sc, a_g, _ = run(ops, route, case, thr=None, tau=tau)
        b_sc, b_g, ct = run(ops, route, case, thr=np.full(C, tau, dtype=np.float32), tau=0.123)      # conf_thresh is not read
        assert np.array_equal(a_sc, b_sc), (route, tau, a_sc, b_sc)                                 # same functions, same order
        ident = R.ROUTES[case[0]]['backward'] == 'identity'
        if route == 'pair_det' or ident:
            assert np.array_equal(a_g, b_g), (route, tau, float(np.abs(a_g - b_g).max()))
        else:
            # run-dependent order of the fp32 atomics between tiles (module docstring): both within the bound of one reference
            name, mode, fn, pp, given = case
            N, _, h, w, H, W, ac = R.geometry(name)
            ref = R.consistency(R.inputs(case), H, W, ac, mode, fn, np.full(C, tau, np.float32), pp, R.RAMP, R.WEIGHT)
            bound = L.grad_bound(ref)
            S.assert_within(a_g, ref['grad'], bound, 'existing')
            S.assert_within(b_g, ref['grad'], bound, 'cthresh')
        assert table(ct)[0] > 0


# ------------------------------------------------------------------------------------------------------------ order independence
@pytest.mark.parametrize('case', [R.CASES[2], R.CASES[3], R.CASES[6], R.CASES[8]], ids=R.case_id)
def test_tables_do_not_depend_on_how_the_batch_is_split(ops, case):
    ref = R.reference(case, 'ascending')
    C = R.geometry(case[0])[1]
    for route in ('pair', 'fused'):
        sc, g, whole = run(ops, route, case, ref['thr'])
        parts = thresholds(ops, ref['thr'])
        for rows in (slice(0, 1), slice(1, 2)):
            run(ops, route, case, ct=parts, rows=rows)
        assert table(parts) == table(whole)
        # the same bits again, and twice the table after a second call into it
        sc2, g2, again = run(ops, route, case, ref['thr'])
        assert table(again) == table(whole) and np.array_equal(sc, sc2)
        run(ops, route, case, ct=again)
        assert table(again) == [2 * v for v in table(whole)]
        # thr after update(): bit for bit
        for ct in (whole, parts):
            ct.update()
        assert torch.equal(whole.thr, parts.thr) and torch.equal(whole.state, parts.state) and table(whole) == [0] * (2 + 3 * C)
        assert torch.equal(whole.epoch, parts.epoch) and int(whole.epoch[0]) == ref['table'][0]
    # backward in samples= runs writes the rows of one backward; the statistics come from the forward launch alone
    sc, g, ct = run(ops, 'pair_det', case, ref['thr'])
    sc3, g3, ct3 = run(ops, 'pair_det', case, ref['thr'], samples=[(0, 1), (1, 2)])
    assert np.array_equal(g, g3) and table(ct) == table(ct3)
    # a non-zero grad_out is added to
    init = np.full(g.shape, 0.25, dtype=np.float32)
    sc4, g4, _ = run(ops, 'pair_det', case, ref['thr'], grad_init=init)
    # (a cell receives one add per tile that touches it -- at most 2 tile columns x 4 tile rows at these scales --, each rounded at
    # the magnitude of what is there, 0.25; the subtraction below is exact)
    S.assert_within(g4 - 0.25, ref['grad'], ref['bound'] + 8 * L.U32 * 0.25, 'accumulated')


@pytest.mark.parametrize('case', [R.CASES[2], R.CASES[7], R.CASES[8]], ids=R.case_id)
def test_dirty_workspace_and_the_autograd_entry(ops, case):
    """The workspace is scratch: whatever it holds on entry, every launch writes the partial sums it reads (tiled, direct-gather and
    identity forward; the fused launch). And ops.consistency_loss, the autograd entry, routes to the class-threshold launches too."""
    from cutmix_semisup_seg_amd._lib import fn as cfn
    name, mode, fn, pp, given = case
    N, C, h, w, H, W, ac = R.geometry(name)
    ref = R.reference(case, 'ascending')
    i = R.inputs(case)
    ct = thresholds(ops, ref['thr'])
    cfg = ops.ConsistencyConfig(mode=mode, loss_fn=fn, conf_per_pixel=pp, align_corners=ac, invert=True, class_thresh=ct)
    ts = [cu(i['ls']), cu(i['l0']), cu(i['l1'])]
    kw = dict(ranges=ops.ranges_to_device(i['ranges'], DEV), um0=cu(i['um0']), um1=cu(i['um1']))
    d = ops._cons_desc(cfg, ts[0], ts[1], ts[2], kw['ranges'], None, kw['um0'], kw['um1'], (H, W))
    cd = ops._ct_desc(cfg, d)
    nbytes = int(cfn['cms_cthresh_workspace_bytes'](ctypes.byref(cd)))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fused = bool(cfn['cms_cthresh_fused_supported'](ctypes.byref(cd)))
    out = []
    for fill in (0x00, 0xA5, 0xFF):                       # 0xFF..: NaNs as floats
        ws = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
        stats = torch.full((4,), float('nan'), dtype=torch.float64, device=DEV)
        ct.table.zero_()
        assert cfn['cms_cthresh_fwd'](ctypes.byref(cd), p(ws), p(stats), st) == 0
        row = [stats.cpu().clone(), table(ct)]
        assert bool((ws[nbytes:] == fill).all())          # and nothing behind what was asked for
        if fused:
            ws.fill_(fill)
            g = torch.zeros_like(ts[0])
            ct.table.zero_()
            assert cfn['cms_cthresh_fwd_bwd'](ctypes.byref(cd), 1.0, p(ws), p(stats), p(g), st) == 0
            row += [stats.cpu().clone(), table(ct)]
            assert bool((ws[nbytes:] == fill).all())
        torch.cuda.synchronize()
        out.append(row)
    for row in out[1:]:
        assert torch.equal(row[0], out[0][0]) and row[1] == out[0][1] and torch.isfinite(row[0]).all()
        if fused:
            assert torch.equal(row[2], out[0][2]) and row[3] == out[0][3] and row[3] == row[1]      # (the table: the same integers)
    check_table(out[0][1], ref, C, 'dirty workspace ' + R.case_id(case))
    # the autograd entry: the scalars of consistency_forward, the gradient of consistency_backward, the table of one forward launch
    with K._Deterministic(ops, True):
        ct.table.zero_()
        sc, ctx = ops.consistency_forward(cfg, *ts, (H, W), ramp_val=R.RAMP, cons_weight=R.WEIGHT, **kw)
        want_g = ops.consistency_backward(ctx, sc)
        want_tab = table(ct)
        ct.table.zero_()
        ls = ts[0].clone().requires_grad_(True)
        unsup, closs, rate = ops.consistency_loss(ls, ts[1], ts[2], (H, W), cfg, ramp_val=R.RAMP, cons_weight=R.WEIGHT, **kw)
        unsup.backward()
        torch.cuda.synchronize()
    assert float(unsup) == float(sc[3]) and float(closs) == float(sc[0]) and float(rate) == float(sc[1])
    assert torch.equal(ls.grad, want_g) and table(ct) == want_tab
    K.check_consistency(sc.cpu().numpy().astype(np.float64), ls.grad.cpu().numpy(), ref, 'autograd ' + R.case_id(case), weight=R.WEIGHT)


# ------------------------------------------------------------------------------------------------------------ update launch
def _state(ct):
    return [float(v) for v in ct.state.cpu().numpy()], [np.float32(v) for v in ct.thr.cpu().numpy()]


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[2], R.CASES[5]], ids=R.case_id)
def test_update_launch_equals_the_restatement_from_its_own_table(ops, case):
    C = R.geometry(case[0])[1]
    for lam, floor, ceil in ((0.5, 0.0, 0.97), (0.999, 0.3, 0.6)):
        ct = ops.ClassThresholds(C, DEV, ema=lam, floor=floor, ceil=ceil)
        st, th = R.initial(C, floor, ceil)
        assert _state(ct) == (st, th)
        ep = [0] * (1 + 2 * C)
        ct.update()                                                   # nothing seen yet: everything as it is
        assert _state(ct) == (st, th)
        for k in range(3):                                            # three updates in a row, thr moving under the forward launches
            run(ops, 'pair' if k % 2 else 'fused', case, ct=ct)
            tab = table(ct)
            assert tab[0] > 0
            st, th, _, ep = R.update(st, th, tab, ep, C, True, lam, floor, ceil)
            ct.update()
            gs, gt = _state(ct)
            assert gs == st, (k, gs, st)
            assert all(abs(float(a) - float(b)) <= R.ulp32(b) for a, b in zip(gt, th)), (k, gt, th)
            th = gt
            assert table(ct) == [0] * (2 + 3 * C)
            assert [int(v) for v in ct.epoch.cpu().numpy()] == ep
        rep = ct.pop_epoch_report()
        assert rep['n_valid'] == ep[0] and rep['pixels'] == ep[1:1 + C] and not ct.epoch.any()
        assert all((r is None) == (p == 0) for r, p in zip(rep['pass_rate'], rep['pixels']))
        assert rep['tau'] == st[0] and np.array_equal(rep['thr'], np.array(th, np.float32))
    # static mode moves only the counters
    lst = [0.5 + 0.4 * c / C for c in range(C)]
    ct = ops.ClassThresholds(C, DEV, mode=lst)
    before = _state(ct)
    assert [float(v) for v in before[1]] == [float(np.float32(v)) for v in lst]
    run(ops, 'pair', case, ct=ct)
    tab = table(ct)
    ct.update()
    assert _state(ct) == before and table(ct) == [0] * (2 + 3 * C)
    assert [int(v) for v in ct.epoch.cpu().numpy()] == [tab[0]] + tab[2 + C:]


# ------------------------------------------------------------------------------------------------------------ refusal
def test_toobig_is_refused_with_the_same_code_and_nothing_touched(ops):
    from cutmix_semisup_seg_amd._lib import fn as cfn
    case = R.REFUSED
    name, mode, fn, pp, given = case
    N, C, h, w, H, W, ac = R.geometry(name)
    i = R.inputs(case)
    ct = thresholds(ops, np.full(C, 0.5, np.float32))
    ct.table.fill_(7)
    cfg = ops.ConsistencyConfig(mode=mode, loss_fn=fn, align_corners=ac, class_thresh=ct)
    ts = [cu(i['ls']), cu(i['l0']), cu(i['l1'])]
    d = ops._cons_desc(cfg, ts[0], ts[1], ts[2], ops.ranges_to_device(i['ranges'], DEV), None, cu(i['um0']), cu(i['um1']), (H, W))
    cd = ops._ct_desc(cfg, d)
    g = torch.full((N, C, h, w), 3.0, device=DEV)
    sc = torch.ones(4, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stats = torch.full((4,), -1.0, dtype=torch.float64, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert cfn['cms_cthresh_fused_supported'](ctypes.byref(cd)) == 0
    want = cfn['cms_consistency_bwd'](ctypes.byref(d), p(sc), p(g), st)
    assert want != 0
    assert cfn['cms_cthresh_bwd'](ctypes.byref(cd), p(sc), p(g), st) == want
    assert cfn['cms_cthresh_fwd_bwd'](ctypes.byref(cd), 1.0, p(ws), p(stats), p(g), st) == cfn['cms_consistency_fwd_bwd'](
        ctypes.byref(d), 1.0, p(ws), p(stats), p(g), st) != 0
    torch.cuda.synchronize()
    assert bool((g == 3.0).all()) and bool((ct.table == 7).all()) and bool((stats == -1.0).all())
    with pytest.raises(ValueError, match='LDS'):
        ctx = ops.consistency_forward(cfg, *ts, (H, W), ranges=ops.ranges_to_device(i['ranges'], DEV), um0=cu(i['um0']), um1=cu(i['um1']))
        ops.consistency_backward(ctx[1], ctx[0], g)
    # (its forward launch -- the direct-gather kernel with 32 run-time classes -- exists and counts)
    ref_rows = R.rows_of(case)
    ct.table.zero_()
    ops.consistency_forward(cfg, *ts, (H, W), ranges=ops.ranges_to_device(i['ranges'], DEV), um0=cu(i['um0']), um1=cu(i['um1']))
    tab = table(ct)
    assert tab[0] == int(ref_rows['valid'].sum())
    assert tab[2 + C:2 + 2 * C] == [int((ref_rows['valid'] & (ref_rows['kstar'] == c)).sum()) for c in range(C)]


# ------------------------------------------------------------------------------------------------------------ the step
STEP = dict(C=5, layers=[1, 1, 1, 1], N=2, H=65, W=65, head_scale=200.0)


def _net(seed, dtype=torch.float32):
    from architectures import deeplab2
    torch.manual_seed(seed)
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, STEP['layers'], STEP['C'], np.zeros(3), np.ones(3))
    # a freshly initialised head gives logits of +-0.01 (every confidence 0.2008): scaled, so that the confidences spread over
    # (0.2, 1) and per-class thresholds have something to decide
    with torch.no_grad():
        for p in net.new_parameters():
            p.mul_(STEP['head_scale'])
    net = net.to(DEV)
    net.compute_dtype = dtype
    net.train()
    net.freeze_batchnorm()
    return net


def _make_step(ops, fuse=True, deterministic=False, class_thresh='freematch', dtype=torch.float32, conf_thresh=0.97):
    from cutmix_semisup_seg_amd import optim as fo
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig
    import optim_weight_ema
    ops.set_deterministic_wgrad(False)
    stu, tea = _net(77, dtype), _net(77, dtype)
    opt = fo.FusedAdam(stu, [dict(params=list(stu.pretrained_parameters()), lr=1e-4), dict(params=list(stu.new_parameters()), lr=1e-3)])
    for p in tea.parameters():
        p.requires_grad = False
    topt = optim_weight_ema.EMAWeightOptimizer(tea, stu, 0.99)
    topt.fuse_into(opt)
    ct = ops.ClassThresholds(STEP['C'], DEV, ema=0.5, floor=0.0, ceil=0.97) if class_thresh == 'freematch' else class_thresh
    cfg = StepConfig(mask_mode='mix', cons_loss_fn='var', conf_thresh=conf_thresh, compute_dtype=dtype, fuse_batches=fuse,
                     deterministic=deterministic, class_thresh=ct)
    return stu, tea, CutMixMeanTeacherStep(stu, tea, opt, topt, cfg), ct


def _data(seed=5):
    g = torch.Generator().manual_seed(seed)
    N, H, W, C = STEP['N'], STEP['H'], STEP['W'], STEP['C']
    d = dict(x=torch.randn(N, 3, H, W, generator=g), y=torch.randint(0, C, (N, H, W), generator=g).to(torch.uint8),
             ux0=torch.randn(N, 3, H, W, generator=g), ux1=torch.randn(N, 3, H, W, generator=g),
             um0=(torch.rand(N, 1, H, W, generator=g) > 0.2).float(), um1=(torch.rand(N, 1, H, W, generator=g) > 0.2).float())
    d['ranges'] = torch.from_numpy(L.boxes(np.random.RandomState(seed), N, H, W, 1))
    return {k: v.to(DEV) for k, v in d.items()}


def _unsup(d):
    from cutmix_semisup_seg_amd.step import UnsupBatch
    return UnsupBatch(d['ux0'], d['ranges'], um0=d['um0'], x1_tea=d['ux1'], um1=d['um1'])


def _restate(ops, stu, tea, d, thr):
    """the iteration's consistency loss restated in fp64 from the device's own logits of the three passes"""
    with torch.no_grad():
        l0, l1 = tea.forward_lowres(d['ux0']).float(), tea.forward_lowres(d['ux1']).float()
        ls = stu.forward_lowres(ops.cutmix_paste(d['ux0'], d['ux1'], ranges=d['ranges'], invert=True)).float()
    i = dict(ls=ls.cpu().numpy(), l0=l0.cpu().numpy(), l1=l1.cpu().numpy(), ranges=d['ranges'].cpu().numpy(), mask=None,
             um0=d['um0'].cpu().numpy(), um1=d['um1'].cpu().numpy())
    return R.consistency(i, STEP['H'], STEP['W'], True, 'mix', 'var', thr, False)


def test_step_two_iterations_in_freematch_mode(ops):
    C, P = STEP['C'], STEP['N'] * STEP['H'] * STEP['W']
    d = _data()
    stu, tea, step, ct = _make_step(ops)
    thr0 = np.full(C, np.float32(1.0 / C))
    assert np.array_equal(ct.thr.cpu().numpy(), thr0)
    want1 = _restate(ops, stu, tea, d, thr0)
    r1 = step(d['x'], d['y'], [_unsup(d)])
    # iteration 1: thr = 1 / C, the largest of C probabilities reaches it: everything passes
    assert float(r1['conf_rate']) == 1.0 and want1['scalars'][1] == 1.0
    assert float(r1['consistency_loss']) == pytest.approx(want1['scalars'][0], rel=1e-4)
    tab = table(ct)
    assert tab[0] == want1['table'][0] and sum(tab[2 + C:2 + 2 * C]) == tab[0] and tab[2 + 2 * C:] == tab[2 + C:2 + 2 * C]
    for k in range(1, 2 + C):                                   # the logits of the step's passes are those of the passes above to ~1e-6
        assert abs(tab[k] - want1['table'][k]) <= want1['table_bound'][k] + 1e-4 * want1['table'][k] + 2 ** 24
    st, th, _, _ = R.update(*R.initial(C, 0.0, 0.97), tab, [0] * (1 + 2 * C), C, True, 0.5, 0.0, 0.97)
    # iteration 2 applies the thresholds made from iteration 1's table
    want2 = _restate(ops, stu, tea, d, np.array(th, np.float32))
    r2 = step(d['x'], d['y'], [_unsup(d)])
    # (the update at the head of iteration 2 ran before its launches; the table now holds iteration 2's sums)
    assert [float(v) for v in ct.state.cpu().numpy()] == st
    assert all(abs(float(a) - float(b)) <= R.ulp32(b) for a, b in zip(ct.thr.cpu().numpy(), th))
    assert len(set(float(v) for v in th)) > 1 and max(th) > np.float32(1.0 / C)                 # the thresholds moved, per class
    close = int((np.abs(want2['conf'] - np.array(th, np.float64)[want2['kstar']]) < 1e-4).sum())
    rate2 = want2['scalars'][1]
    print('iteration 2: rate', float(r2['conf_rate']), 'restated', rate2, 'pixels within 1e-4 of their threshold', close)
    assert abs(float(r2['conf_rate']) - rate2) <= (close + 0.5) / P
    assert float(r2['consistency_loss']) == pytest.approx(want2['scalars'][0], rel=1e-4 + (close + 0.5) / P / rate2)
    assert table(ct)[0] == want2['table'][0]


def test_step_routes_agree(ops, monkeypatch):
    d = _data()
    out = {}
    for route in ('fused', 'separate', 'graphed'):
        monkeypatch.setenv('CMS_STEP_GRAPH', '1' if route == 'graphed' else '0')
        stu, tea, step, ct = _make_step(ops, fuse=route == 'fused')
        res = [step(d['x'], d['y'], [_unsup(d)]) for _ in range(4 if route == 'graphed' else 2)]       # (two eager iterations, then replay)
        torch.cuda.synchronize()
        thr = ct.thr.cpu().numpy().copy()
        ct.update()                                                   # fold the last iteration's table into the epoch counters
        out[route] = ([{k: float(v) for k, v in r.items()} for r in res], thr, ct.pop_epoch_report())
    for route in ('separate', 'graphed'):
        for a, b in zip(out['fused'][0][:2], out[route][0][:2]):
            assert a['conf_rate'] == pytest.approx(b['conf_rate'], abs=5e-4)
            assert a['consistency_loss'] == pytest.approx(b['consistency_loss'], rel=2e-3)
            assert a['sup_loss'] == pytest.approx(b['sup_loss'], rel=1e-4)
    assert out['graphed'][2]['n_valid'] == 2 * out['fused'][2]['n_valid']                       # the replayed launches counted too
    assert all(np.isfinite(list(r.values())).all() for r in out['graphed'][0])


def _deterministic_run(ops, d, dtype, iters):
    """`iters` iterations under StepConfig(deterministic=True) -> per iteration (the three scalars, the integer table the iteration
    left), then thr, the fp64 state, the epoch counters and the student's parameters"""
    stu, tea, step, ct = _make_step(ops, deterministic=True, dtype=dtype)
    per = []
    for _ in range(iters):
        r = step(d['x'], d['y'], [_unsup(d)])
        torch.cuda.synchronize()
        per.append((torch.stack([r[k] for k in ('sup_loss', 'consistency_loss', 'conf_rate')]).cpu(), ct.table.cpu().clone()))
    return per, ct.thr.cpu(), ct.state.cpu(), ct.epoch.cpu(), [p.detach().cpu().clone() for p in stu.parameters()]


def test_deterministic_step_reproduces_itself_bit_for_bit(ops):
    """StepConfig(deterministic=True) with class thresholds, two runs from the same start.
    bf16 passes -- the configuration tests/test_gpu_determinism.py holds --deterministic to: EVERYTHING repeats bit for bit over three
    iterations: the scalars, the integer tables, thr, the fp64 state (tau, p~), the epoch counters, the student's weights.
    fp32 passes -- the configuration the other step tests run in: the fp32 weight gradient (cms_conv_wgrad_f32) always joins its pixel
    slices with fp32 atomics; ops.conv_wgrad gives the deterministic slab route to bf16 only. So in fp32 the student's weights, and
    with them the teacher's and every later logit, differ run to run from the first optimizer step on, with or without class
    thresholds. What class thresholds add must still repeat: the first iteration's scalars and integer table -- made by
    forward passes of identical weights --, and the state and thr the update at the head of the second iteration makes from that
    table alone."""
    d = _data()
    db = {k: (v.bfloat16() if k in ('x', 'ux0', 'ux1') else v) for k, v in d.items()}
    try:
        a, b = _deterministic_run(ops, db, torch.bfloat16, 3), _deterministic_run(ops, db, torch.bfloat16, 3)
        for (sa, ta), (sb, tb) in zip(a[0], b[0]):
            assert torch.equal(sa, sb) and torch.equal(ta, tb)
        assert int(a[0][0][1].sum()) > 0                                                           # (the tables hold something)
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])     # thr, state, epoch counters
        assert len(set(float(v) for v in a[1])) > 1                                              # ... of thresholds that moved
        differing = [i for i, (x, y) in enumerate(zip(a[4], b[4])) if not torch.equal(x, y)]
        assert not differing, differing
        a, b = _deterministic_run(ops, d, torch.float32, 2), _deterministic_run(ops, d, torch.float32, 2)
        assert torch.equal(a[0][0][0], b[0][0][0]) and torch.equal(a[0][0][1], b[0][0][1])         # iteration 1: scalars and table
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])     # thr, state, epoch: from that table
        print('fp32: student tensors differing after two iterations', sum(1 for x, y in zip(a[4], b[4]) if not torch.equal(x, y)),
              'of', len(a[4]), '; iteration-2 scalars equal', torch.equal(a[0][1][0], b[0][1][0]))
    finally:
        ops.set_deterministic_wgrad(False)


def test_step_without_class_thresh_is_the_parent(ops):
    """class_thresh=None: no cms_cthresh_* entry point is called during the step, and the step's consistency scalars are bit for bit
    those of cms_consistency_fwd_bwd + cms_consistency_finalize called directly through a descriptor filled here, field by field,
    with none of the class-threshold plumbing in between"""
    from cutmix_semisup_seg_amd import _lib
    d = _data()
    tau = 0.3                           # (a threshold some pixels of this network pass: the gradient is not all zero)
    stu, tea, step, _ = _make_step(ops, class_thresh=None, conf_thresh=tau)
    assert step.cfg.cons.class_thresh is None
    seen = {}
    orig = ops.consistency_fused
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def spy(cfg, l_stu, l0, l1, out_size, grad_out, ranges=None, mask=None, um0=None, um1=None, ramp_val=1.0, cons_weight=1.0, **kw):
        n, c, h, w = (int(v) for v in l_stu.shape)
        ts = [t.float().contiguous() for t in (l_stu, l0, l1)]
        cd = _lib.ConsistencyDesc()
        cd.l_stu, cd.l_tea0, cd.l_tea1 = (t.data_ptr() for t in ts)
        cd.ranges, cd.mask, cd.um0, cd.um1 = ranges.data_ptr(), None, um0.data_ptr(), um1.data_ptr()
        cd.n, cd.c, cd.h, cd.w, cd.H, cd.W = n, c, h, w, int(out_size[0]), int(out_size[1])
        cd.align_corners, cd.n_boxes, cd.invert, cd.mode, cd.loss_fn = 1, int(ranges.shape[1]), 1, _lib.MODE_MIX, _lib.LOSS_IDS['var']
        cd.conf_thresh, cd.conf_per_pixel = tau, 0
        assert _lib.fn['cms_consistency_fused_supported'](ctypes.byref(cd)) == 1
        ws = torch.empty(int(_lib.fn['cms_consistency_workspace_bytes'](ctypes.byref(cd))), dtype=torch.uint8, device=DEV)
        stats = torch.empty(4, dtype=torch.float64, device=DEV)
        g = torch.zeros_like(ts[0])
        sc = torch.empty(4, device=DEV)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        unit = float(ramp_val) * float(cons_weight) / float(n * cd.H * cd.W)
        assert _lib.fn['cms_consistency_fwd_bwd'](ctypes.byref(cd), unit, p(ws), p(stats), p(g), st) == 0
        assert _lib.fn['cms_consistency_finalize'](p(stats), p(stats), tau, 0, float(ramp_val), float(cons_weight), p(sc), st) == 0
        got = orig(cfg, l_stu, l0, l1, out_size, grad_out, ranges=ranges, mask=mask, um0=um0, um1=um1, ramp_val=ramp_val,
                   cons_weight=cons_weight, **kw)
        seen['pair'] = (sc.clone(), got.clone(), cfg, g * sc[1], grad_out.clone())
        return got

    def refuse(name):
        def f(*a, **k):
            raise AssertionError('{} was called with class_thresh=None'.format(name))
        return f
    names = [k for k in _lib.fn if k.startswith('cms_cthresh_')]
    assert len(names) == 6
    kept = {k: _lib.fn[k] for k in names}
    ops.consistency_fused = spy
    for k in names:
        _lib.fn[k] = refuse(k)
    try:
        res = step(d['x'], d['y'], [_unsup(d)])
        torch.cuda.synchronize()
    finally:
        ops.consistency_fused = orig
        _lib.fn.update(kept)
    direct, sc, cfg, g_direct, g_step = seen['pair']
    assert cfg.class_thresh is None and cfg.conf_thresh == tau and float(sc[1]) > 0.0
    assert torch.equal(direct, sc) and float(res['consistency_loss']) == float(sc[0]) and float(res['conf_rate']) == float(sc[1])
    # (the gradient's tiles meet in fp32 atomics whose order changes from launch to launch: equal to rounding, not to the bit)
    assert float((g_direct - g_step).abs().max()) <= 1e-5 * float(g_step.abs().max()) and float(g_step.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize('mode', ['freematch', 'static'])
def test_trainer_cli_synthetic_end_to_end(tmp_path, monkeypatch, mode):
    from click.testing import CliRunner
    from cutmix_semisup_seg_amd import checkpoint
    import train_seg_semisup_classthresh_mt as trainer
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = ['--job_desc', 'ct', '--synthetic', '--synthetic_n_classes', '5', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn',
            '--batch_size', '2', '--crop_size', '65,65', '--learning_rate', '3e-5', '--num_epochs', '2', '--iters_per_epoch', '3',
            '--synthetic_val_batches', '1', '--save_model']
    args += ['--thresh_ema', '0.5'] if mode == 'freematch' else ['--class_thresh', '0.3,0.25,0.2,0.4,0.35']
    res = CliRunner().invoke(trainer.experiment, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    run_dir = tmp_path / 'results' / 'train_seg_semisup_classthresh_mt'
    lines = open(run_dir / 'log_ct.txt').read().splitlines()
    epochs = [k for k, l in enumerate(lines) if l.startswith('Epoch ')]
    assert len(epochs) == 2
    num = r'\d\.\d{3}'
    thr = [l for l in lines if l.startswith('-- class thresholds')]
    rate = [l for l in lines if l.startswith('-- class pass rate')]
    assert len(thr) == 2 and len(rate) == 2
    for l in thr:
        assert re.match(r'-- class thresholds tau={n}: {n}(, {n}){{4}}$'.format(n=num), l), l
    for l in rate:
        assert re.match(r'-- class pass rate (-|[\d.]+%)(, (-|[\d.]+%)){4}$', l), l
    where = [k for k, l in enumerate(lines) if l.startswith('-- class thresholds')]
    assert where[0] > epochs[0] and where[1] > epochs[1] > where[0]                              # behind each epoch's own lines
    if mode == 'static':
        assert thr[0].endswith(': 0.300, 0.250, 0.200, 0.400, 0.350') and thr[0] == thr[1]
    else:
        assert thr[0] != thr[1] or 'tau=0.200' not in thr[1]
    assert (run_dir / 'ct' / 'model.pth').exists()
    net = checkpoint.load_model(str(run_dir / 'ct' / 'model.pth'))            # eval_seg's loader
    assert net.state_dict()['conv1.weight'].shape[1] == 3
