"""
GPU: the augmentation-consistency path -- the fused affine-warp loss (cms_aug_fwd / cms_aug_bwd behind
ops.aug_consistency_forward / _backward), AugMeanTeacherStep and the trainer -- against tests/_aug_refs.py, the torch
restatement of train_seg_semisup_aug_mt.py:302-397 (F.affine_grid / F.grid_sample / autograd on the CPU).

Tolerances of the loss comparisons are the project's own for this arithmetic (tests/test_hostcheck.py::
test_consistency_with_upsample_vs_oracle, the same as tests/test_aug_hostcheck.py): loss rel 2e-5, rate abs 2e-6, gradient
rtol 5e-4 with atol 5e-6 * max|want|.

The confidence threshold is discontinuous. Every thresholded case asserts, on the CPU reference, that NO pixel's warped
confidence lies within 1e-5 of tau (tau = 0.6, teacher logits scaled x3); the seeds in GEOS were searched on the CPU for that
(first seed from 0 upwards with a margin of 5e-5) and are not special otherwise. No pixel is skipped anywhere.
"""
import re

import numpy as np
import pytest
import torch

import _aug_refs as refs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAU = 0.6
MODES = {'default': (TAU, False), 'per_pixel': (TAU, True), 'no_thresh': (0.0, False)}
R = refs.rot_scale_theta

# Per-sample warps of three kinds: a small rotation + translation, a strong rotation + scale, and one that pushes a large part
# of the view outside (zero padding, wholly outside tiles). Tiles of the loss kernels: 64 columns; 8 rows forward, 4 backward.
#   tiles      70 x 150 from 9 x 19: 3 tile columns (64 + 64 + 22), partial last tile rows (6 of 8, 2 of 4), compile-time
#              C = 21, both align_corners; the teacher's rectangle is staged in LDS
#   c5 / c7    41 x 50 from 6 x 7: one partial tile column, compile-time C = 5 and run-time C = 7
#   ident      h == H, w == W (the U-Nets): the direct kernels without upsampling, C = 2
#   fallback   64 x 64 from 60 x 60 with 21 classes, 45 degrees: the teacher's rectangle of a tile exceeds the capacity, the
#              taps are gathered from global memory (tests/test_aug_cpu.py asserts the route of every geometry here)
#   direct_rt  64 x 64 from 60 x 60 with 46 (run-time) classes: the student's forward rectangle (46 x 9 x 62 floats = 100 KB)
#              exceeds the 96 KB limit of the LDS-staged forward, which then gathers from global memory; the backward runs
#              with 147 KB of LDS and 9 KB left for the teacher's rectangle. Four samples: 46 classes leave few confident pixels
#   ident_rt   the identity kernels with a run-time class count, C = 3
THREE = [R(8, 1.0, 0.06, -0.04), R(-33, 1.3, 0.0, 0.0), R(12, 0.9, 0.8, -0.7)]
GEOS = {
    'tiles_align': dict(N=3, C=21, lo=(9, 19), hi=(70, 150), ac=True, theta=THREE, seed=29),
    'tiles_noalign': dict(N=3, C=21, lo=(9, 19), hi=(70, 150), ac=False, theta=THREE, seed=8),
    'c5': dict(N=3, C=5, lo=(6, 7), hi=(41, 50), ac=True, theta=THREE, seed=7),
    'c7': dict(N=3, C=7, lo=(6, 7), hi=(41, 50), ac=False, theta=THREE, seed=2),
    'ident': dict(N=2, C=2, lo=(24, 40), hi=(24, 40), ac=True, theta=[R(8, 1.0, 0.06, -0.04), R(-33, 1.3, 0.6, -0.5)], seed=1),
    'fallback': dict(N=2, C=21, lo=(60, 60), hi=(64, 64), ac=True, theta=[R(45, 1.0), R(45, 1.2, 0.7, 0.6)], seed=0),
    'direct_rt': dict(N=4, C=46, lo=(60, 60), hi=(64, 64), ac=True, theta=THREE + [R(45, 1.2, 0.7, 0.6)], seed=3),
    'ident_rt': dict(N=2, C=3, lo=(24, 40), hi=(24, 40), ac=True, theta=[R(8, 1.0, 0.06, -0.04), R(-33, 1.3, 0.6, -0.5)], seed=0),
}
ALL_LOSSES_AT = ('tiles_align', 'tiles_noalign', 'c5')


def make_inputs(geo):
    N, C, (h, w), (H, W) = geo['N'], geo['C'], geo['lo'], geo['hi']
    gen = torch.Generator().manual_seed(geo['seed'])
    ls = torch.randn(N, C, h, w, generator=gen) * 2
    lt = torch.randn(N, C, h, w, generator=gen) * 3
    um0 = (torch.rand(N, 1, H, W, generator=gen) > 0.3).float()
    um1 = (torch.rand(N, 1, H, W, generator=gen) > 0.3).float()
    return ls, lt, um0, um1, torch.tensor(geo['theta'], dtype=torch.float32)


def min_margin(geo, tau=TAU):
    """smallest |warped confidence - tau| of a geometry on the CPU (the seed search)"""
    _, lt, _, _, theta = make_inputs(geo)
    conf = refs.warped_confidence(refs.upsample(lt, geo['hi'], align_corners=geo['ac']), theta)
    return float((conf - tau).abs().min())


_CACHE = {}
_REFS = {}


def inputs(name):
    """CPU tensors and their device copies, made once per geometry and never modified"""
    if name not in _CACHE:
        cpu = make_inputs(GEOS[name])
        _CACHE[name] = (cpu, tuple(t.to(DEV) for t in cpu))
    return _CACHE[name]


def reference(name, fn, mode, ramp=0.7, weight=0.3):
    """the CPU restatement of one case, computed once and shared"""
    key = (name, fn, mode, ramp, weight)
    if key not in _REFS:
        geo = GEOS[name]
        tau, pp = MODES[mode]
        ls, lt, um0, um1, theta = inputs(name)[0]
        wm = mode != 'no_thresh'
        _REFS[key] = refs.aug_from_lowres(ls, lt, theta, um0 if wm else None, um1 if wm else None, geo['hi'], geo['ac'],
                                          cons_loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, ramp_val=ramp, rampup=5,
                                          cons_weight=weight)
    return _REFS[key]


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


def _assert_clear_of_threshold(conf, tau):
    assert float((conf - tau).abs().min()) > 1e-5, 'a pixel sits on the threshold: pick another seed'


def _device_loss(ops, dev, geo, fn, tau, pp, ramp, weight, with_masks=True, grad_out=None, force_global=False, theta=None,
                 l_tea=None, um0='own', um1='own'):
    ls, lt, m0, m1, th = dev
    cfg = ops.AugConsistencyConfig(loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=geo['ac'], force_global=force_global)
    m0 = (m0 if with_masks else None) if isinstance(um0, str) else um0
    m1 = (m1 if with_masks else None) if isinstance(um1, str) else um1
    sc, ctx = ops.aug_consistency_forward(cfg, ls, lt if l_tea is None else l_tea, th if theta is None else theta, geo['hi'],
                                          um0=m0, um1=m1, ramp_val=ramp, cons_weight=weight)
    grad = ops.aug_consistency_backward(ctx, sc, grad_out)
    return sc.cpu().numpy(), grad.cpu(), ctx


CASES = [(name, fn) for name in sorted(GEOS) for fn in refs.LOSS_FNS if fn in ('var', 'kld') or name in ALL_LOSSES_AT]


# ---------------------------------------------------------------------------------------------------------------- loss kernels
@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name,fn', CASES, ids=['{}-{}'.format(*c) for c in CASES])
def test_aug_loss_kernels_vs_reference_restatement(ops, name, fn, mode):
    geo = GEOS[name]
    tau, pp = MODES[mode]
    _, dev = inputs(name)
    with_masks = mode != 'no_thresh'                       # um0 / um1 random in {0,1}; the NULL (= all ones) path without a threshold
    ramp, weight = 0.7, 0.3
    r, want, conf = reference(name, fn, mode, ramp, weight)
    if tau > 0:
        _assert_clear_of_threshold(conf, tau)
        # both sides of the threshold are populated: at least 100 pixels each (21 blended classes leave few confident pixels)
        assert min(r['conf_rate'], 1.0 - r['conf_rate']) * conf.numel() >= 100
    sc, grad, _ = _device_loss(ops, dev, geo, fn, tau, pp, ramp, weight, with_masks)
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
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(grad.numpy(), want, rtol=5e-4, atol=5e-6 * np.abs(want).max())


@pytest.mark.parametrize('mode', ['default', 'per_pixel'])
@pytest.mark.parametrize('fn', ['var', 'logits_smoothl1'])
@pytest.mark.parametrize('name', ['tiles_align', 'tiles_noalign', 'c5', 'c7', 'fallback'])
def test_staged_and_global_routes_give_the_same_bits(ops, name, fn, mode):
    """the teacher's rectangle in LDS against the descriptor's force_global: the same bilin_gather on the same values"""
    geo = GEOS[name]
    tau, pp = MODES[mode]
    _, dev = inputs(name)
    with _Deterministic(ops):
        s_a, g_a, ctx_a = _device_loss(ops, dev, geo, fn, tau, pp, 0.7, 0.3)
        s_b, g_b, ctx_b = _device_loss(ops, dev, geo, fn, tau, pp, 0.7, 0.3, force_global=True)
    assert torch.equal(ctx_a[3], ctx_b[3])                 # the double[4] statistics
    assert np.array_equal(s_a, s_b, equal_nan=True) and torch.equal(g_a, g_b)
    assert float(g_a.abs().max()) > 0


def _identity(n):
    return torch.tensor([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]] * n)


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('fn', refs.LOSS_FNS)
@pytest.mark.parametrize('name', ['c5', 'tiles_align', 'ident'])
def test_identity_warp_is_the_cut_mode_consistency(ops, name, fn, mode):
    """An exact identity matrix samples every teacher pixel with one tap of weight 1: loss, rate and gradient are those of the
    existing fused kernel in cut mode with an all-ones box mask, um1 = 1 and the same um0, within the tolerances of the reference
    comparison (`kld` takes log of the warped probability where the existing kernel uses the logit form)."""
    geo = GEOS[name]
    tau, pp = MODES[mode]
    cpu, dev = inputs(name)
    ls, lt, um0, _, _ = dev
    N = geo['N']
    if tau > 0:
        _assert_clear_of_threshold(refs.warped_confidence(refs.upsample(cpu[1], geo['hi'], align_corners=geo['ac']), _identity(N)), tau)
    cons_cfg = ops.ConsistencyConfig(mode='cut', loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, align_corners=geo['ac'],
                                     invert=False)
    ones = torch.zeros((N, 1, 4), dtype=torch.int32, device=DEV)      # an empty box, not inverted: the all-ones mask
    with _Deterministic(ops):
        sc_a, g_a, _ = _device_loss(ops, dev, geo, fn, tau, pp, 0.7, 0.3, theta=_identity(N), um0=um0, um1=None)
        sc_c, ctx_c = ops.consistency_forward(cons_cfg, ls, lt, None, geo['hi'], ranges=ones, um0=um0, ramp_val=0.7, cons_weight=0.3)
        g_c = ops.consistency_backward(ctx_c, sc_c)
    sc_c, g_a, g_c = sc_c.cpu().numpy(), g_a.numpy(), g_c.cpu().numpy()
    assert sc_a[0] == pytest.approx(sc_c[0], rel=2e-5) and sc_a[3] == pytest.approx(sc_c[3], rel=2e-5)
    if tau > 0:
        assert sc_a[1] == pytest.approx(sc_c[1], abs=2e-6)
    np.testing.assert_allclose(g_a, g_c, rtol=5e-4, atol=5e-6 * np.abs(g_c).max())


@pytest.mark.parametrize('fn', ['var', 'logits_var'])
@pytest.mark.parametrize('name', ['c5', 'tiles_noalign', 'ident'])
def test_half_turn_of_the_teacher_is_the_identity_on_the_flipped_teacher(ops, name, fn):
    """theta = -I maps pixel (x, y) to (W-1-x, H-1-y) exactly: the same as the identity on l_tea and um0 flipped in both axes
    (the upsample commutes with the flip up to the rounding of its weights: the tolerances of the reference comparison)"""
    geo = GEOS[name]
    cpu, dev = inputs(name)
    N = geo['N']
    _assert_clear_of_threshold(refs.warped_confidence(refs.upsample(cpu[1], geo['hi'], align_corners=geo['ac']), _identity(N)), TAU)
    with _Deterministic(ops):
        sc_a, g_a, _ = _device_loss(ops, dev, geo, fn, TAU, True, 0.7, 0.3, theta=-_identity(N))
        sc_b, g_b, _ = _device_loss(ops, dev, geo, fn, TAU, True, 0.7, 0.3, theta=_identity(N),
                                    l_tea=torch.flip(dev[1], (2, 3)).contiguous(), um0=torch.flip(dev[2], (2, 3)).contiguous())
    assert sc_a[0] == pytest.approx(sc_b[0], rel=2e-5) and sc_a[1] == pytest.approx(sc_b[1], abs=2e-6)
    np.testing.assert_allclose(g_a.numpy(), g_b.numpy(), rtol=5e-4, atol=5e-6 * float(g_b.abs().max()))
    assert float(g_a.abs().max()) > 0


@pytest.mark.parametrize('name', ['c5', 'tiles_align', 'ident'])
def test_missing_um0_is_the_zero_padded_ones_mask(ops, name):
    """(the third warp of these geometries leaves a large part of the view outside)"""
    geo = GEOS[name]
    _, dev = inputs(name)
    ones = torch.ones_like(dev[2])
    with _Deterministic(ops):
        s_a, g_a, _ = _device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0, um0=None)
        s_b, g_b, _ = _device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0, um0=ones)
    assert np.array_equal(s_a, s_b) and torch.equal(g_a, g_b)


def test_aug_backward_accumulates_into_a_given_gradient(ops):
    geo = GEOS['c5']
    _, dev = inputs('c5')
    _, g, _ = _device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0)
    init = torch.full_like(dev[0], 0.25)
    _, g2, _ = _device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0, grad_out=init)
    # (every add into a cell that holds 0.25 rounds at half an ulp of 0.25 = 2^-26; a cell receives a handful of tile sums)
    torch.testing.assert_close(g2 - 0.25, g, rtol=0, atol=1e-6 * float(g.abs().max()) + 8 * 2.0 ** -26)


@pytest.mark.parametrize('mode', ['default', 'per_pixel'])
def test_aug_backward_is_reproducible_in_deterministic_mode(ops, mode):
    geo = GEOS['tiles_align']
    _, dev = inputs('tiles_align')
    tau, pp = MODES[mode]
    with _Deterministic(ops):
        (s1, g1, _), (s2, g2, _) = (_device_loss(ops, dev, geo, 'var', tau, pp, 1.0, 1.0) for _ in range(2))
    assert np.array_equal(s1, s2) and torch.equal(g1, g2)
    assert float(g1.abs().max()) > 0


def test_xf_is_accepted_as_numpy_cpu_and_device_tensor(ops):
    geo = GEOS['c5']
    _, dev = inputs('c5')
    th = inputs('c5')[0][4]
    with _Deterministic(ops):
        outs = [_device_loss(ops, dev, geo, 'var', TAU, False, 1.0, 1.0, theta=t) for t in (th.numpy(), th, th.to(DEV))]
    for s, g, _ in outs[1:]:
        assert np.array_equal(s, outs[0][0]) and torch.equal(g, outs[0][1])


def test_wrapper_errors(ops):
    geo = GEOS['c5']
    (ls, lt, um0, um1, th), dev = inputs('c5')
    cfg = ops.AugConsistencyConfig()
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, ls, lt, th, geo['hi'])                        # CPU logits
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1][:, :4], th, geo['hi'])         # shape mismatch
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1], th[:2], geo['hi'])            # one matrix short
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1], th.reshape(3, 6), geo['hi'])  # not (N,2,3)
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1], th, geo['hi'], um0=dev[2][:, :, :40])   # mask of the wrong size
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1], th, geo['hi'], um1=dev[3][:2])
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1], th, (1, 50))                  # H < 2
    with pytest.raises(ValueError):
        ops.aug_consistency_forward(cfg, dev[0], dev[1], th, (4, 5))                   # logits larger than the loss geometry
    with pytest.raises(ValueError, match='Unknown consistency loss function'):
        ops.AugConsistencyConfig(loss_fn='l2')
    sc, ctx = ops.aug_consistency_forward(cfg, dev[0], dev[1], th, geo['hi'])
    with pytest.raises(ValueError):
        ops.aug_consistency_backward(ctx, sc, torch.zeros(3, 5, 6, 8, device=DEV))


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


# tau: the randomly initialised network's warped confidences are zero outside the teacher's view and 0.2 .. 0.3 inside; this is
# the middle of the widest gap between two neighbouring pixels' values in the central half of the inside values for this seed
# (found on the CPU: 5.4e-5 to either side). cons_weight: the consistency value of a random network is ~5e-4 against a cross
# entropy of 1.6; x 100 lets its gradient count in the weights that are compared
STEP = dict(C=5, layers=[1, 1, 1, 1], N=2, H=33, W=41, theta=[R(10, 1.1, 0.05, -0.05), R(-20, 0.9, 0.1, 0.0)], seed=11,
            tau=0.2565839, alpha=0.99, lr=1.0, cons_weight=100.0)
STEP_KEYS = ('conv1.weight', 'layer3.0.conv2.weight', 'layer5.conv2d_list.1.weight')


def _step_data():
    g = torch.Generator().manual_seed(STEP['seed'])
    N, C, H, W = STEP['N'], STEP['C'], STEP['H'], STEP['W']
    x = torch.randn(N, 3, H, W, generator=g)
    y = torch.randint(0, C, (N, 1, H, W), generator=g)
    y[torch.rand(N, 1, H, W, generator=g) < 0.05] = 255
    ux0, ux1 = torch.randn(N, 3, H, W, generator=g), torch.randn(N, 3, H, W, generator=g)
    um0 = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
    um1 = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
    return x, y, ux0, ux1, um0, um1, torch.tensor(STEP['theta'], dtype=torch.float32)


def _make_step(st, dtype, cfg, sgd=False):
    from cutmix_semisup_seg_amd import aug, optim as fo
    import optim_weight_ema
    stu, tea = _net(STEP['C'], STEP['layers'], st, dtype), _net(STEP['C'], STEP['layers'], st, dtype)
    groups = [dict(params=list(stu.pretrained_parameters()), lr=STEP['lr'] * 0.1), dict(params=list(stu.new_parameters()), lr=STEP['lr'])]
    opt = fo.FusedSGD(stu, groups) if sgd else fo.FusedAdam(stu, [dict(g, lr=g['lr'] * 1e-2) for g in groups])
    for p in tea.parameters():
        p.requires_grad = False
    ema = optim_weight_ema.EMAWeightOptimizer(tea, stu, STEP['alpha'])
    ema.fuse_into(opt)
    return stu, tea, aug.AugMeanTeacherStep(stu, tea, opt, ema, cfg)


def test_aug_step_matches_the_cpu_restatement_of_the_iteration():
    """One AugMeanTeacherStep call in fp32 against the iteration restated on the CPU: oracle.deeplab2 for the network passes,
    tests/_aug_refs.py for the warp and the loss, autograd for the gradients. Student and teacher start from the same weights.
    Plain SGD (no momentum, no decay) so that the student's weights after the step are w - lr * gradient and compare linearly.
    Tolerance: the ICT step test's 1e-4 -- for the gradients relative to the tensor's largest element as well (a weight gradient
    is a long sum with cancellation: its absolute error scales with the large terms); for the weights after the step the same on
    the update, plus one float32 spacing of the weights themselves."""
    from oracle import deeplab2 as odl, losses as olosses
    from cutmix_semisup_seg_amd import aug
    st = _state(STEP['C'], STEP['layers'])
    x, y, ux0, ux1, um0, um1, theta = _step_data()
    st_s = dict(st)
    for k in STEP_KEYS:
        st_s[k] = st[k].clone().requires_grad_(True)
    fnet = lambda t, s: odl.forward(t, s, STEP['layers'], frozen=True)
    with torch.no_grad():
        LT = fnet(ux0, st)
    sup = olosses.supervised_ce(fnet(x, st_s), y[:, 0].long())
    r = refs.aug_unsup_loss(fnet(ux1, st_s), LT, theta, um0, um1, cons_loss_fn='var', conf_thresh=STEP['tau'], conf_per_pixel=False,
                            cons_weight=STEP['cons_weight'])
    (sup + r['unsup_loss']).backward()
    conf = refs.warped_confidence(LT, theta)
    # a pixel that changes sides moves the rate by 1 / (N*H*W) = 3.7e-4: the fp32 rounding of the network passes (1e-6 of a
    # probability) must stay well inside the gap around tau
    assert float((conf - STEP['tau']).abs().min()) > 4e-5
    assert 0.1 < r['conf_rate'] < 0.9

    cfg = aug.AugConfig(cons_loss_fn='var', cons_weight=STEP['cons_weight'], conf_thresh=STEP['tau'])
    stu, tea, step = _make_step(st, torch.float32, cfg, sgd=True)
    t0 = {k: v.clone() for k, v in tea.state_dict().items() if v.dtype == torch.float32}
    ub = aug.AugUnsupBatch(ux0.to(DEV), ux1.to(DEV), theta.numpy(), um0=um0.to(DEV), um1=um1.to(DEV))
    res = step(x.to(DEV), y.to(DEV).to(torch.uint8), [ub])
    got = {k: float(v) for k, v in res.items()}
    print('step:', got, 'want', float(sup.detach()), float(r['consistency_loss'].detach()), r['conf_rate'])
    assert got['sup_loss'] == pytest.approx(float(sup.detach()), rel=1e-4)
    assert got['consistency_loss'] == pytest.approx(float(r['consistency_loss'].detach()), rel=1e-4)
    assert got['conf_rate'] == pytest.approx(r['conf_rate'], rel=1e-4)
    sd_s, sd_t = stu.state_dict(), tea.state_dict()
    params = dict(stu.named_parameters())
    mult = {}
    for grp in odl.param_multiplicity(STEP['C'], STEP['layers']):
        mult.update(grp)
    assert [mult[k] for k in STEP_KEYS] == [1, 3, 1]
    for k in STEP_KEYS:
        lr = STEP['lr'] * (1.0 if k.startswith('layer5') else 0.1)
        g_want = st_s[k].grad
        g_got = params[k].grad.detach().float().cpu()           # (the optimizer's gradient arena, cleared by the next step)
        gmax = float(g_want.abs().max())
        print(k, 'max|grad|', gmax, 'max|grad diff|', float((g_got - g_want).abs().max()))
        assert gmax > 1e-4
        torch.testing.assert_close(g_got, g_want, rtol=1e-4, atol=1e-4 * gmax)
        # the reference's pretrained_parameters() yields a backbone weight once per enclosing module (oracle.deeplab2.
        # param_multiplicity: 3 for a bottleneck convolution), and the optimizer updates it that many times per step
        m = mult[k]
        w_want = st[k] - m * lr * g_want
        torch.testing.assert_close(sd_s[k].cpu(), w_want, rtol=0,
                                   atol=m * (2e-4 * lr * gmax + 2.0 ** -23 * float(st[k].abs().max())))
        torch.testing.assert_close(sd_t[k], t0[k] * STEP['alpha'] + sd_s[k] * (1.0 - STEP['alpha']), rtol=1e-5, atol=1e-7)


def test_aug_step_bf16_pi_model_and_batch_ratio():
    """bf16 run of the same step: finite losses, the student moves; teacher is student (the Pi model) with two unsupervised
    batches per iteration (--unsup_batch_ratio 2), a ramp-up and no threshold."""
    from cutmix_semisup_seg_amd import aug, optim as fo
    st = _state(STEP['C'], STEP['layers'])
    x, y, ux0, ux1, um0, um1, theta = _step_data()
    cfg = aug.AugConfig(cons_loss_fn='var', cons_weight=1.0, conf_thresh=STEP['tau'])
    stu, tea, step = _make_step(st, torch.bfloat16, cfg)
    s0 = {k: v.clone() for k, v in stu.state_dict().items() if v.dtype == torch.float32}
    b = lambda t: t.to(DEV).bfloat16()
    res = step(b(x), y.to(DEV).to(torch.uint8), [aug.AugUnsupBatch(b(ux0), b(ux1), theta, um0=um0.to(DEV), um1=um1.to(DEV))])
    vals = {k: float(v) for k, v in res.items()}
    assert all(np.isfinite(v) for v in vals.values()) and vals['consistency_loss'] > 0, vals
    assert any(not torch.equal(s0[k], v) for k, v in stu.state_dict().items() if k in s0)

    pi = _net(STEP['C'], STEP['layers'], st, torch.float32)
    opt = fo.FusedAdam(pi, [dict(params=list(pi.pretrained_parameters()), lr=1e-4), dict(params=list(pi.new_parameters()), lr=1e-3)])
    pstep = aug.AugMeanTeacherStep(pi, pi, opt, None, aug.AugConfig(cons_loss_fn='logits_var', conf_thresh=0.0, rampup=5, unsup_batch_ratio=2))
    ubs = [aug.AugUnsupBatch(ux0.to(DEV), ux1.to(DEV), theta.to(DEV)), aug.AugUnsupBatch(ux1.to(DEV), ux0.to(DEV), theta)]
    res = pstep(x.to(DEV), y.to(DEV).to(torch.uint8), ubs, ramp_val=0.5)
    assert np.isfinite(float(res['sup_loss'])) and float(res['consistency_loss']) > 0 and np.isnan(float(res['conf_rate']))


# ---------------------------------------------------------------------------------------------------------------- trainer
def test_aug_trainer_cli_synthetic_end_to_end(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_aug_mt as trainer
    monkeypatch.chdir(tmp_path)
    args = ['--job_desc', 'aug', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2',
            '--crop_size', '65,65', '--learning_rate', '3e-5', '--aug_rot_mag', '20', '--aug_max_scale', '1.3', '--aug_hflip',
            '--conf_thresh', '0.97', '--num_epochs', '1', '--iters_per_epoch', '2', '--synthetic_val_batches', '1']
    res = CliRunner().invoke(trainer.experiment, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    log = open(tmp_path / 'results' / 'train_seg_semisup_aug_mt' / 'log_aug.txt').read()
    lines = [l for l in log.splitlines() if l.startswith('Epoch ')]
    assert len(lines) == 1
    assert re.match(r'Epoch \d+: took [\d.]+s, TRAIN clf loss=[\d.]+, consistency loss=[\d.]+, conf rate=[\d.]+%, '
                    r'VAL mIoU=[\d.]+%', lines[0]), lines
