"""
GPU: the ICT (interpolation consistency training) path -- cms_ict_blend, the fused interpolation loss (cms_ict_fwd / cms_ict_bwd
behind ops.ict_consistency_forward / _backward), ICTMeanTeacherStep and the trainer -- against tests/_ict_refs.py, the torch
restatement of train_seg_semisup_ict.py:306-391 (which builds the --conf_per_pixel mask with the reference's literal
(N,N,1,H,W) broadcast, so the kernels' batch-mean form is what gets tested).

Tolerances of the loss comparisons are the project's own for this arithmetic (tests/test_hostcheck.py::
test_consistency_with_upsample_vs_oracle, the same as tests/test_ict_hostcheck.py): loss rel 2e-5, rate abs 2e-6, gradient
rtol 5e-4 with atol 5e-6 * max|want|.

The confidence threshold is discontinuous. Every thresholded case asserts, on the CPU reference, that NO pixel's blended
confidence lies within 1e-5 of tau (tau = 0.6, logits scaled x3); the seeds in GEOS / STEP were searched on the CPU for that
(first seed from 1 upwards with a margin of 5e-5) and are not special otherwise. No pixel is skipped anywhere.
"""
import re

import numpy as np
import pytest
import torch

import _ict_refs as refs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAU = 0.6
MODES = {'default': (TAU, False), 'per_pixel': (TAU, True), 'no_thresh': (0.0, False)}

# Tiles of the loss kernels (csrc/loss_tiles.hpp): TILE_W = 64 columns; 8 rows in the forward, 4 in the backward.
#   tiles      70 x 150 from 9 x 19: 3 tile columns (64 + 64 + 22) x 9 forward / 18 backward tile rows, the last ones partial
#              (6 of 8 and 2 of 4 rows), compile-time C = 21, both align_corners
#   c5 / c7    41 x 50 from 6 x 7: one partial tile column, compile-time C = 5 and run-time C = 7
#   ident      h == H, w == W (the U-Nets): the direct kernels without upsampling, C = 2
#   direct     64 x 64 from 60 x 60 with 21 classes: the forward rectangles (3 x 21 x 9 x 62 floats = 140 KB) exceed the 96 KB limit
#              of the LDS-staged forward, which then gathers from global memory; the backward runs with 120 KB of LDS
#   direct_rt  the same route with a run-time class count: one sample, C = 16 (3 x 16 x 9 x 62 floats = 105 KB)
#   ident_rt   the identity kernels with a run-time class count, C = 3
#              (tests/test_ict_cpu.py asserts the route of every geometry here)
GEOS = {
    'tiles_align': dict(N=3, C=21, lo=(9, 19), hi=(70, 150), ac=True, lam=[0.0, 1.0, 0.37], seed=56),
    'tiles_noalign': dict(N=3, C=21, lo=(9, 19), hi=(70, 150), ac=False, lam=[0.81, 0.05, 0.5], seed=14),
    'c5': dict(N=3, C=5, lo=(6, 7), hi=(41, 50), ac=True, lam=[0.0, 1.0, 0.37], seed=7),
    'c7': dict(N=3, C=7, lo=(6, 7), hi=(41, 50), ac=False, lam=[0.37, 0.0, 1.0], seed=1),
    'ident': dict(N=2, C=2, lo=(24, 40), hi=(24, 40), ac=True, lam=[0.0, 0.63], seed=6),
    'direct': dict(N=2, C=21, lo=(60, 60), hi=(64, 64), ac=True, lam=[1.0, 0.2], seed=1),
    'direct_rt': dict(N=1, C=16, lo=(60, 60), hi=(64, 64), ac=True, lam=[0.37], seed=0),
    'ident_rt': dict(N=2, C=3, lo=(24, 40), hi=(24, 40), ac=True, lam=[0.0, 0.63], seed=0),
}


def make_inputs(geo):
    N, C, (h, w), (H, W) = geo['N'], geo['C'], geo['lo'], geo['hi']
    gen = torch.Generator().manual_seed(geo['seed'])
    ls = torch.randn(N, C, h, w, generator=gen) * 2
    l0 = torch.randn(N, C, h, w, generator=gen) * 3
    l1 = torch.randn(N, C, h, w, generator=gen) * 3
    um0 = (torch.rand(N, 1, H, W, generator=gen) > 0.3).float()
    um1 = (torch.rand(N, 1, H, W, generator=gen) > 0.3).float()
    return ls, l0, l1, um0, um1, torch.tensor(geo['lam'], dtype=torch.float32)


_CACHE = {}


def inputs(name):
    """CPU tensors and their device copies, made once per geometry and never modified"""
    if name not in _CACHE:
        cpu = make_inputs(GEOS[name])
        _CACHE[name] = (cpu, tuple(t.to(DEV) for t in cpu))
    return _CACHE[name]


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops
    return ops


class _Deterministic(object):
    """cms_loss_set_deterministic(1) for the block, the session's setting restored behind it"""

    def __init__(self, ops):
        from cutmix_semisup_seg_amd._lib import fn
        self.fn, self.ops = fn, ops

    def __enter__(self):
        self.fn['cms_loss_set_deterministic'](1)

    def __exit__(self, *exc):
        self.fn['cms_loss_set_deterministic'](1 if self.ops.deterministic_wgrad() else 0)


# ---------------------------------------------------------------------------------------------------------------- blend
@pytest.mark.parametrize('shape', [(3, 3, 5, 7), (4, 1, 6, 9), (2, 3, 33, 41), (5, 1, 1, 3), (2, 3, 8, 16)],
                         ids=lambda s: 'x'.join(str(v) for v in s))
def test_blend_matches_the_torch_expression(ops, shape):
    """fp32: bit-equal to x0*(1-lam) + x1*lam evaluated by torch on the device in fp32; bf16: that fp32 result rounded once.
    chw = 105, 54 (a mask: chw = H*W), 4059 and 3 are no multiples of the vector width (4 fp32 / 8 bf16 elements), so vectors
    straddle sample boundaries and a scalar tail remains; 384 is a multiple of both."""
    gen = torch.Generator().manual_seed(sum(shape))
    x0, x1 = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
    lam = torch.rand(shape[0], generator=gen).to(DEV)
    f = lam.reshape(-1, 1, 1, 1)
    want = x0 * (1.0 - f) + x1 * f
    got = ops.ict_blend(x0, x1, lam)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(ops.ict_blend(x0, x1, f), want)                     # the reference's (N,1,1,1) factors
    b0, b1 = x0.bfloat16(), x1.bfloat16()
    want16 = (b0.float() * (1.0 - f) + b1.float() * f).bfloat16()
    got16 = ops.ict_blend(b0, b1, lam)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, want16)
    # views that start off a 16-byte boundary take the element-wise kernel
    flat0, flat1 = torch.zeros(x0.numel() + 1, device=DEV), torch.zeros(x0.numel() + 1, device=DEV)
    flat0[1:], flat1[1:] = x0.reshape(-1), x1.reshape(-1)
    assert torch.equal(ops.ict_blend(flat0[1:].reshape(shape), flat1[1:].reshape(shape), lam), want)


def test_blend_with_lambda_zero_and_one_returns_the_inputs(ops):
    gen = torch.Generator().manual_seed(9)
    x0, x1 = torch.randn(4, 3, 5, 7, generator=gen).to(DEV), torch.randn(4, 3, 5, 7, generator=gen).to(DEV)
    lam = torch.tensor([0.0, 1.0, 0.0, 1.0], device=DEV)
    for a, b in ((x0, x1), (x0.bfloat16(), x1.bfloat16())):
        out = ops.ict_blend(a, b, lam)
        assert torch.equal(out[0], a[0]) and torch.equal(out[2], a[2])
        assert torch.equal(out[1], b[1]) and torch.equal(out[3], b[3])
    with pytest.raises(ValueError):
        ops.ict_blend(x0, x1, lam[:3])


# ---------------------------------------------------------------------------------------------------------------- loss kernels
def _assert_clear_of_threshold(conf, tau):
    assert float((conf - tau).abs().min()) > 1e-5, 'a pixel sits on the threshold: pick another seed'


def _device_loss(ops, dev, geo, fn, tau, pp, ramp, weight, with_masks=True, grad_out=None):
    ls, l0, l1, um0, um1, lam = dev
    cfg = ops.ICTConsistencyConfig(loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=geo['ac'])
    sc, ctx = ops.ict_consistency_forward(cfg, ls, l0, l1, lam, geo['hi'], um0=um0 if with_masks else None,
                                          um1=um1 if with_masks else None, ramp_val=ramp, cons_weight=weight)
    grad = ops.ict_consistency_backward(ctx, sc, grad_out)
    return sc.cpu().numpy(), grad.cpu()


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('fn', refs.LOSS_FNS)
@pytest.mark.parametrize('name', sorted(GEOS))
def test_ict_loss_kernels_vs_reference_restatement(ops, name, fn, mode):
    geo = GEOS[name]
    tau, pp = MODES[mode]
    (ls, l0, l1, um0, um1, lam), dev = inputs(name)
    with_masks = mode != 'no_thresh'                       # um0 / um1 random in {0,1}; the NULL (= all ones) path without a threshold
    ramp, weight = 0.7, 0.3
    r, want, conf = refs.ict_from_lowres(ls, l0, l1, lam, um0 if with_masks else None, um1 if with_masks else None, geo['hi'],
                                         geo['ac'], cons_loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, ramp_val=ramp, rampup=5,
                                         cons_weight=weight)
    if tau > 0:
        _assert_clear_of_threshold(conf, tau)
        assert 0.02 < r['conf_rate'] < 0.98                # both sides of the threshold are populated
    sc, grad = _device_loss(ops, dev, geo, fn, tau, pp, ramp, weight, with_masks)
    closs, unsup = float(r['consistency_loss'].detach()), float(r['unsup_loss'].detach())
    print('{} {} {}: loss {:.9g} vs {:.9g}, rate {} vs {}, max|grad diff| / max|grad| {:.3g}'.format(
        name, fn, mode, sc[0], closs, sc[1], r['conf_rate'], float((grad - want).abs().max() / want.abs().max())))
    assert sc[0] == pytest.approx(closs, rel=2e-5)
    assert sc[3] == pytest.approx(unsup, rel=2e-5)
    if tau > 0:
        assert sc[1] == pytest.approx(r['conf_rate'], abs=2e-6)
    else:
        assert np.isnan(sc[1])
    want = want.numpy()
    np.testing.assert_allclose(grad.numpy(), want, rtol=5e-4, atol=5e-6 * np.abs(want).max())


def test_ict_backward_accumulates_into_a_given_gradient(ops):
    geo = GEOS['c5']
    _, dev = inputs('c5')
    _, g = _device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0)
    init = torch.full_like(dev[0], 0.25)
    _, g2 = _device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0, grad_out=init)
    # (every add into a cell that holds 0.25 rounds at half an ulp of 0.25 = 2^-26; a cell receives a handful of tile sums)
    torch.testing.assert_close(g2 - 0.25, g, rtol=0, atol=1e-6 * float(g.abs().max()) + 8 * 2.0 ** -26)


# ---------------------------------------------------------------------------------------------------------------- cross-check
@pytest.mark.parametrize('mode,name', [('default', 'c5'), ('no_thresh', 'c5'), ('default', 'tiles_align'), ('per_pixel', 'one')])
@pytest.mark.parametrize('fn', refs.LOSS_FNS)
@pytest.mark.parametrize('which', [0, 1], ids=['lam0', 'lam1_swapped'])
def test_ict_with_lambda_zero_is_the_cut_mode_consistency(ops, which, fn, mode, name):
    """lambda == 0 (and lambda == 1 with the teachers swapped) blends nothing: loss, rate and gradient are those of the existing
    fused kernel in cut mode with an all-ones box mask (the VAT usage). `kld` takes log of the blended probability where the
    existing kernel uses the logit form: the tolerances of the reference comparison. For the other four losses the formulas
    coincide term by term and the gradients agree to 1e-6 of the gradient's largest element (the measure of
    tests/test_gpu_parity.py::test_loss_backward_one_launch_equals_colour_classes), both in the reproducible tile order.
    --conf_per_pixel coincides for N = 1 only, where the batch mean of the indicator is the sample's own."""
    if name == 'one':
        geo = dict(GEOS['c7'], N=1, lam=[0.0], seed=3)
        cpu = make_inputs(geo)
        dev = tuple(t.to(DEV) for t in cpu)
    else:
        geo = GEOS[name]
        cpu, dev = inputs(name)
    tau, pp = MODES[mode]
    ls, l0, l1, um0, um1, _ = dev
    if tau > 0:
        _assert_clear_of_threshold(refs.blended_confidence(refs.upsample(cpu[1], geo['hi'], geo['ac']),
                                                           refs.upsample(cpu[1], geo['hi'], geo['ac']), [0.0] * geo['N']), tau)
    N = geo['N']
    lam = torch.full((N,), float(which), device=DEV)
    ict_cfg = ops.ICTConsistencyConfig(loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=geo['ac'])
    cons_cfg = ops.ConsistencyConfig(mode='cut', loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=geo['ac'],
                                     invert=False)
    ones = torch.zeros((N, 1, 4), dtype=torch.int32, device=DEV)      # an empty box, not inverted: the all-ones mask
    with _Deterministic(ops):
        # the teacher that counts is l0 with its mask um0; the other one carries weight exactly zero
        a = (l0, l1, um0, um1) if which == 0 else (l1, l0, um1, um0)
        sc_i, ctx_i = ops.ict_consistency_forward(ict_cfg, ls, a[0], a[1], lam, geo['hi'], um0=a[2], um1=a[3], ramp_val=0.7,
                                                  cons_weight=0.3)
        g_i = ops.ict_consistency_backward(ctx_i, sc_i)
        sc_c, ctx_c = ops.consistency_forward(cons_cfg, ls, l0, None, geo['hi'], ranges=ones, um0=um0, ramp_val=0.7, cons_weight=0.3)
        g_c = ops.consistency_backward(ctx_c, sc_c)
    sc_i, sc_c, g_i, g_c = sc_i.cpu().numpy(), sc_c.cpu().numpy(), g_i.cpu().numpy(), g_c.cpu().numpy()
    assert sc_i[0] == pytest.approx(sc_c[0], rel=2e-5) and sc_i[3] == pytest.approx(sc_c[3], rel=2e-5)
    if tau > 0:
        assert sc_i[1] == pytest.approx(sc_c[1], abs=2e-6)
    np.testing.assert_allclose(g_i, g_c, rtol=5e-4, atol=5e-6 * np.abs(g_c).max())
    if fn != 'kld':
        assert np.abs(g_i - g_c).max() <= 1e-6 * np.abs(g_c).max()


# ---------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize('mode', ['default', 'per_pixel'])
def test_ict_backward_is_reproducible_in_deterministic_mode(ops, mode):
    geo = GEOS['tiles_align']
    _, dev = inputs('tiles_align')
    tau, pp = MODES[mode]
    with _Deterministic(ops):
        (s1, g1), (s2, g2) = (_device_loss(ops, dev, geo, 'var', tau, pp, 1.0, 1.0) for _ in range(2))
    assert np.array_equal(s1, s2) and torch.equal(g1, g2)
    assert float(g1.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- step
def _state(C, layers):
    """random, non-degenerate weights and BatchNorm statistics (the recipe of tests/test_gpu_vat.py)"""
    from oracle import deeplab2 as odl
    g = torch.Generator().manual_seed(77)
    st = {}
    for k, (shape, dt) in odl.state_spec(C, layers).items():
        if dt == torch.int64:
            st[k] = torch.zeros(shape, dtype=torch.int64)
        elif len(shape) == 4:
            st[k] = torch.randn(shape, generator=g) * (1.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith('running_var'):
            st[k] = 0.8 + 0.4 * torch.rand(shape, generator=g)
        elif k.endswith('running_mean'):
            st[k] = 0.1 * torch.randn(shape, generator=g)
        elif k.endswith('.weight'):
            st[k] = 0.6 + 0.8 * torch.rand(shape, generator=g)
        else:
            st[k] = 0.1 * torch.randn(shape, generator=g)
    return st


def _net(C, layers, st, dtype):
    from architectures import deeplab2
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, layers, C, np.zeros(3), np.ones(3))
    net.load_state_dict(st)
    net = net.to(DEV)
    net.compute_dtype = dtype
    net.train()
    net.freeze_batchnorm()
    return net


# tau: the randomly initialised network's blended confidences lie in 0.22 .. 0.31; this is the middle of the widest gap between two
# neighbouring pixels' values in the central half of that distribution for this seed (5.7e-5 to either side, found on the CPU)
STEP = dict(C=5, layers=[1, 1, 1, 1], N=2, H=33, W=41, lam=[0.3, 0.85], seed=11, tau=0.26108779, alpha=0.99)


def _step_data():
    g = torch.Generator().manual_seed(STEP['seed'])
    N, C, H, W = STEP['N'], STEP['C'], STEP['H'], STEP['W']
    x = torch.randn(N, 3, H, W, generator=g)
    y = torch.randint(0, C, (N, 1, H, W), generator=g)
    y[torch.rand(N, 1, H, W, generator=g) < 0.05] = 255
    ux0, ux1 = torch.randn(N, 3, H, W, generator=g), torch.randn(N, 3, H, W, generator=g)
    um0 = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
    um1 = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
    return x, y, ux0, ux1, um0, um1


def _make_step(st, dtype, cfg):
    from cutmix_semisup_seg_amd import ict, optim as fo
    import optim_weight_ema
    stu, tea = _net(STEP['C'], STEP['layers'], st, dtype), _net(STEP['C'], STEP['layers'], st, dtype)
    opt = fo.FusedAdam(stu, [dict(params=list(stu.pretrained_parameters()), lr=1e-4), dict(params=list(stu.new_parameters()), lr=1e-3)])
    for p in tea.parameters():
        p.requires_grad = False
    ema = optim_weight_ema.EMAWeightOptimizer(tea, stu, STEP['alpha'])
    ema.fuse_into(opt)
    return stu, tea, ict.ICTMeanTeacherStep(stu, tea, opt, ema, cfg)


def test_ict_step_matches_the_cpu_restatement_of_the_iteration():
    """One ICTMeanTeacherStep call in fp32 with injected mix factors against the iteration restated on the CPU: oracle.deeplab2 for
    the three network passes, tests/_ict_refs.py for the blend and the loss. Student and teacher start from the same weights."""
    from oracle import deeplab2 as odl, losses as olosses
    from cutmix_semisup_seg_amd import ict
    st = _state(STEP['C'], STEP['layers'])
    x, y, ux0, ux1, um0, um1 = _step_data()
    lam = torch.tensor(STEP['lam'])
    fnet = lambda t: odl.forward(t, st, STEP['layers'], frozen=True)
    with torch.no_grad():
        want_sup = float(olosses.supervised_ce(fnet(x), y[:, 0].long()))
        L0, L1 = fnet(ux0), fnet(ux1)
        r = refs.ict_unsup_loss(fnet(refs.blend(ux0, ux1, lam)), L0, L1, lam, um0, um1, cons_loss_fn='var', conf_thresh=STEP['tau'],
                                conf_per_pixel=False, cons_weight=0.3)
    # a pixel that changes sides moves the rate by 1 / (N*H*W) = 3.7e-4 (1e-3 of the rate): the fp32 rounding of the network
    # passes (1e-6 of a probability) must stay well inside the gap around tau
    assert float((refs.blended_confidence(L0, L1, lam) - STEP['tau']).abs().min()) > 4e-5
    assert 0.1 < r['conf_rate'] < 0.9

    cfg = ict.ICTConfig(ict_alpha=0.1, cons_loss_fn='var', cons_weight=0.3, conf_thresh=STEP['tau'])
    stu, tea, step = _make_step(st, torch.float32, cfg)
    s0 = {k: v.clone() for k, v in stu.state_dict().items() if v.dtype == torch.float32}
    t0 = {k: v.clone() for k, v in tea.state_dict().items() if v.dtype == torch.float32}
    ub = ict.ICTUnsupBatch(ux0.to(DEV), ux1.to(DEV), um0=um0.to(DEV), um1=um1.to(DEV))
    res = step(x.to(DEV), y.to(DEV).to(torch.uint8), [ub], lam=lam.to(DEV))
    got = {k: float(v) for k, v in res.items()}
    print('step:', got, 'want', want_sup, float(r['consistency_loss']), r['conf_rate'])
    assert got['sup_loss'] == pytest.approx(want_sup, rel=1e-4)
    assert got['consistency_loss'] == pytest.approx(float(r['consistency_loss']), rel=1e-4)
    assert got['conf_rate'] == pytest.approx(r['conf_rate'], rel=1e-4)
    sd_s, sd_t = stu.state_dict(), tea.state_dict()
    assert any(not torch.equal(s0[k], sd_s[k]) for k in s0)
    for k in ('conv1.weight', 'layer3.0.conv2.weight', 'layer5.conv2d_list.1.weight'):
        torch.testing.assert_close(sd_t[k], t0[k] * STEP['alpha'] + sd_s[k] * (1.0 - STEP['alpha']), rtol=1e-5, atol=1e-7)


def test_ict_step_bf16_and_pi_model():
    """bf16 run of the same step: finite losses, the student moves; a draw of its own (no injected factors); teacher is student
    (the Pi model) works as in the other steps."""
    from cutmix_semisup_seg_amd import ict, optim as fo
    st = _state(STEP['C'], STEP['layers'])
    x, y, ux0, ux1, um0, um1 = _step_data()
    cfg = ict.ICTConfig(ict_alpha=0.1, cons_loss_fn='var', cons_weight=0.3, conf_thresh=STEP['tau'])
    stu, tea, step = _make_step(st, torch.bfloat16, cfg)
    step.rng = np.random.RandomState(4)
    s0 = {k: v.clone() for k, v in stu.state_dict().items() if v.dtype == torch.float32}
    b = lambda t: t.to(DEV).bfloat16()
    res = step(b(x), y.to(DEV).to(torch.uint8), [ict.ICTUnsupBatch(b(ux0), b(ux1), um0=um0.to(DEV), um1=um1.to(DEV))])
    vals = {k: float(v) for k, v in res.items()}
    assert all(np.isfinite(v) for v in vals.values()) and vals['consistency_loss'] > 0, vals
    assert any(not torch.equal(s0[k], v) for k, v in stu.state_dict().items() if k in s0)

    pi = _net(STEP['C'], STEP['layers'], st, torch.float32)
    opt = fo.FusedAdam(pi, [dict(params=list(pi.pretrained_parameters()), lr=1e-4), dict(params=list(pi.new_parameters()), lr=1e-3)])
    pstep = ict.ICTMeanTeacherStep(pi, pi, opt, None, ict.ICTConfig(cons_loss_fn='var', conf_thresh=0.0, rampup=5),
                                   rng=np.random.RandomState(5))
    res = pstep(x.to(DEV), y.to(DEV).to(torch.uint8), [ict.ICTUnsupBatch(ux0.to(DEV), ux1.to(DEV))], ramp_val=0.5)
    assert np.isfinite(float(res['sup_loss'])) and float(res['consistency_loss']) > 0 and np.isnan(float(res['conf_rate']))


# ---------------------------------------------------------------------------------------------------------------- trainer
def test_ict_trainer_cli_synthetic_end_to_end(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_ict as trainer
    monkeypatch.chdir(tmp_path)
    args = ['--job_desc', 'ict', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2',
            '--crop_size', '65,65', '--learning_rate', '3e-5', '--ict_alpha', '0.1', '--conf_thresh', '0.97', '--num_epochs', '1',
            '--iters_per_epoch', '2', '--synthetic_val_batches', '1']
    res = CliRunner().invoke(trainer.experiment, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    log = open(tmp_path / 'results' / 'train_seg_semisup_ict' / 'log_ict.txt').read()
    lines = [l for l in log.splitlines() if l.startswith('Epoch ')]
    assert len(lines) == 1
    assert re.match(r'Epoch \d+: took [\d.]+s, TRAIN clf loss=[\d.]+, consistency loss=[\d.]+, conf rate=[\d.]+%, '
                    r'VAL mIoU=[\d.]+%', lines[0]), lines
