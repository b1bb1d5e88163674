"""
GPU: CowMask made on the device (csrc/cowmask.hip through ops.cowmask and mask_gen.CowMaskGenerator), the mask's route through the
step, and the CowMix / CowOut command.

The oracle is the definition restated in numpy float64 (tests/_cowmask_refs.py). The device arithmetic is fp64 from the f32 noise
onward, so its smoothed plane differs from the oracle's by reordering error (~1e-16) while no pixel of these inputs lies closer than
1e-9 to its threshold: the masks must be EQUAL, pixel for pixel.
"""
import os
import re

import numpy as np
import pytest
import torch

import _cowmask_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def oracle():
    """case -> (inputs, mask, stats, margin), computed once and left unchanged"""
    out = {}
    for ci in R.CASES:
        inp = R.case_inputs(ci)
        out[ci] = (inp,) + R.cowmask(inp['noise'], inp['taps'], inp['factor'])
    return out


def _run(ops, inp, with_stats=True):
    noise = torch.from_numpy(inp['noise'])[:, None].to(DEV)
    stats = torch.full((noise.shape[0], 2), float('nan'), dtype=torch.float64, device=DEV) if with_stats else None
    mask = ops.cowmask(noise, inp['taps'], inp['factor'], stats=stats)
    torch.cuda.synchronize()
    return mask, stats


@pytest.mark.parametrize('ci', sorted(R.CASES))
def test_mask_equals_the_fp64_oracle_pixel_for_pixel(ops, oracle, ci):
    inp, want_mask, want_stats, margin = oracle[ci]
    print('\ncase', ci, R.CASES[ci], 'radius', inp['radius'], 'min |s - tau| =', margin)
    assert margin >= 1e-9
    mask, stats = _run(ops, inp)
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (len(inp['p']), 1) + inp['noise'].shape[1:]
    got_stats = stats.cpu().numpy()
    print('stats error', np.abs(got_stats - want_stats).max(), 'differing pixels', int((mask.cpu().numpy() != want_mask).sum()))
    assert torch.equal(mask.cpu(), torch.from_numpy(want_mask))
    assert np.all(np.abs(got_stats - want_stats) <= 1e-12 * (1.0 + np.abs(want_stats)))


@pytest.mark.parametrize('ci', sorted(R.CASES))
def test_sample_alone_equals_sample_in_batch_and_runs_repeat(ops, oracle, ci):
    inp = oracle[ci][0]
    mask, stats = _run(ops, inp)
    again, stats_again = _run(ops, inp)
    assert torch.equal(mask, again) and torch.equal(stats, stats_again)            # the same bits on every run
    for i in range(len(inp['p'])):
        one = dict(noise=inp['noise'][i:i + 1], taps=inp['taps'][i:i + 1], factor=inp['factor'][i:i + 1])
        m1, s1 = _run(ops, one)
        assert torch.equal(m1[0], mask[i]) and torch.equal(s1[0], stats[i]), i


def test_generator_on_the_device(ops, oracle):
    """mask_gen.CowMaskGenerator.torch_masks_from_params: the oracle's mask from [p, sigma] and the caller's noise; its own noise
    from a seeded device generator repeats; out= / no stats"""
    from cutmix_semisup_seg_amd import mask_gen
    inp, want_mask = oracle[3][0], oracle[3][1]
    gen = mask_gen.CowMaskGenerator((0.2, 0.8), (4.0, 16.0))
    params = np.stack([inp['p'], inp['sigma']], axis=1)
    noise = torch.from_numpy(inp['noise'])[:, None].to(DEV)
    got = gen.torch_masks_from_params(params, inp['noise'].shape[1:], torch.device(DEV), noise=noise)
    assert torch.equal(got.cpu(), torch.from_numpy(want_mask))
    g = torch.Generator(device=DEV).manual_seed(12345)
    a = gen.torch_masks_from_params(params, (65, 65), torch.device(DEV), generator=g)
    g.manual_seed(12345)
    b = gen.torch_masks_from_params(params, (65, 65), torch.device(DEV), generator=g)
    assert torch.equal(a, b) and tuple(a.shape) == (2, 1, 65, 65)
    assert set(a.unique().tolist()) <= {0.0, 1.0}
    share = a.mean(dim=(1, 2, 3)).cpu().numpy()
    print('\nshare of ones', share, 'p', inp['p'])
    assert np.all(share > 0.0) and np.all(share < 1.0)


def test_degenerate_inputs(ops):
    from cutmix_semisup_seg_amd import mask_gen
    gen = mask_gen.CowMaskGenerator((0.0, 1.0), (1.0, 3.0))
    dev = torch.device(DEV)
    noise = torch.randn(3, 1, 20, 45, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    m = gen.torch_masks_from_params(np.array([[0.0, 2.0], [1.0, 2.0], [0.5, 2.0]]), (20, 45), dev, noise=noise)
    assert float(m[0].max()) == 0.0 and float(m[1].min()) == 1.0                   # p = 0: all zeros, p = 1: all ones
    assert 0.0 < float(m[2].mean()) < 1.0
    zeros = gen.torch_masks_from_params(np.array([[0.3, 1.0], [0.7, 3.0]]), (20, 45), dev, noise=torch.zeros(2, 1, 20, 45, device=DEV))
    assert float(zeros.min()) == 1.0                                               # 0 <= 0
    one = gen.torch_masks_from_params(np.array([[0.5, 2.0]]), (1, 1), dev, noise=torch.ones(1, 1, 1, 1, device=DEV))
    assert tuple(one.shape) == (1, 1, 1, 1) and float(one) in (0.0, 1.0)
    with pytest.raises(ValueError):
        ops.cowmask(noise, np.ones((3, 4)), np.zeros(3))                           # an even number of taps
    with pytest.raises(ValueError):
        ops.cowmask(noise, np.ones((2, 5)), np.zeros(3))                           # taps of another batch size


# ------------------------------------------------------------------------------------------------------------------ step
def _deeplab_iteration(mask_mode, fuse_batches, as_mask):
    """one iteration of the step on a [1,1,1,1]-block DeepLab v2, deterministic weight gradients -> (scalars, student gradients)"""
    from cutmix_semisup_seg_amd import ops, optim as fo
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig, UnsupBatch
    from architectures import deeplab2
    import mask_gen
    import optim_weight_ema
    C, N, H, W = 5, 2, 65, 65
    torch.manual_seed(3)
    mk = lambda: deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], C, np.zeros(3), np.ones(3)).to(DEV)
    stu, tea = mk(), mk()
    # the fresh networks' logits are ~1e-5 and the consistency term with them: He-initialised convolutions (the frozen BatchNorms are
    # the identity), different for the two networks, put it and its gradient at the size of the supervised ones, where a wrong mask
    # could not hide in the rounding of their sum
    with torch.no_grad():
        for net, seed in ((stu, 21), (tea, 22)):
            gw = torch.Generator().manual_seed(seed)
            for p in net.parameters():
                if p.dim() == 4:
                    fan_in = p.shape[1] * p.shape[2] * p.shape[3]
                    p.copy_((torch.randn(p.shape, generator=gw) * (2.0 / fan_in) ** 0.5).to(p.device))
    opt = fo.FusedAdam(stu, [dict(params=list(stu.pretrained_parameters()), lr=1e-5), dict(params=list(stu.new_parameters()), lr=1e-4)])
    for p in tea.parameters():
        p.requires_grad = False
    ema = optim_weight_ema.EMAWeightOptimizer(tea, stu, 0.99)
    ema.fuse_into(opt)
    stu.train(); tea.train()
    stu.freeze_batchnorm(); tea.freeze_batchnorm()
    stu.engine_kind = tea.engine_kind = 'hip'
    step = CutMixMeanTeacherStep(stu, tea, opt, ema, StepConfig(mask_mode=mask_mode, conf_thresh=0.2, deterministic=True,
                                                              fuse_batches=fuse_batches))
    g = torch.Generator(device=DEV).manual_seed(11)
    im = lambda: torch.randn(N, 3, H, W, generator=g, device=DEV).bfloat16()
    y = torch.randint(0, C, (N, 1, H, W), generator=g, device=DEV).to(torch.uint8)
    ranges = ops.ranges_to_device(mask_gen.BoxMaskGenerator(0.5, invert=True).generate_ranges(N, (H, W), rng=np.random.RandomState(5)), DEV)
    x, u0, u1 = im(), im(), im()
    how = dict(mask=ops.boxmask_rasterize(ranges, (H, W), True)) if as_mask else dict(ranges=ranges)
    try:
        res = step(x, y, [UnsupBatch(u0, x1_tea=u1 if mask_mode == 'mix' else None, **how)])
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic_wgrad(False)
    grads = {k: p.grad.detach().clone() for k, p in stu.named_parameters() if p.grad is not None}
    return {k: float(v) for k, v in res.items()}, grads


@pytest.mark.parametrize('fuse_batches', [True, False], ids=['fused', 'separate'])
@pytest.mark.parametrize('mask_mode', ['mix', 'zero'])
def test_step_with_a_mask_equals_step_with_ranges(mask_mode, fuse_batches):
    """UnsupBatch(mask=the rasterised boxes) against UnsupBatch(ranges=the boxes): paste and teacher selection are exact for a 0/1
    mask and the weight gradients are deterministic, so -- as tests/test_gpu_parity.py::test_cutmix_paste_exact and
    tests/test_gpu_loss_kernels.py::test_box_ranges_and_the_equivalent_float_mask have it for the kernels -- the two are EQUAL."""
    from cutmix_semisup_seg_amd.step import UnsupBatch
    with pytest.raises(ValueError):
        UnsupBatch(torch.zeros(1), ranges=torch.zeros(1), mask=torch.zeros(1))
    res_r, g_r = _deeplab_iteration(mask_mode, fuse_batches, False)
    res_m, g_m = _deeplab_iteration(mask_mode, fuse_batches, True)
    print('\n', mask_mode, 'fused' if fuse_batches else 'separate', 'ranges', res_r, 'mask', res_m)
    assert set(res_r) >= {'sup_loss', 'consistency_loss', 'conf_rate'}
    assert all(np.isfinite(v) for v in res_r.values()) and res_r['consistency_loss'] > 1e-4
    assert res_m == res_r
    assert set(g_m) == set(g_r) and len(g_r) > 10
    differing = [k for k in g_r if not torch.equal(g_r[k], g_m[k])]
    assert not differing, differing[:8]


def test_graph_replayed_separate_passes_take_the_mask():
    """The ResNet-50 U-Net of tests/test_gpu_unets.py::test_cutmix_step_separate_passes_as_hipgraph_match_eager_launches, graphed, fed
    boxes as ranges, the same again (the yardstick) and as materialised masks: new inputs and new masks on every iteration, so the
    replays read the static mask buffer. Where the two ranges runs repeat bit for bit the mask run must equal them; where they do not
    (fp32 atomics reorder from run to run) it may differ from them as that test lets graph and eager runs differ."""
    from architectures import network_architectures
    from cutmix_semisup_seg_amd import ops, optim as fo
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig, UnsupBatch
    import mask_gen
    import optim_weight_ema
    B, H, W, C = 2, 64, 96, 2
    g = torch.Generator(device=DEV).manual_seed(1)
    rng = np.random.RandomState(5)
    data = []
    for _ in range(4):
        y = (torch.rand(B, 1, H, W, generator=g, device=DEV) < 0.4).to(torch.uint8)
        x = (torch.randn(B, 3, H, W, generator=g, device=DEV) + 1.5 * y.float()).bfloat16()
        x0 = torch.randn(B, 3, H, W, generator=g, device=DEV).bfloat16()
        x1 = torch.randn(B, 3, H, W, generator=g, device=DEV).bfloat16()
        r = ops.ranges_to_device(mask_gen.BoxMaskGenerator(0.5, invert=True).generate_ranges(B, (H, W), rng=rng), torch.device(DEV))
        data.append((x, y, x0, x1, r))

    def run(as_mask):
        torch.manual_seed(0)
        Net = network_architectures.seg.get('resnet50unet_imagenet')
        stu, tea = Net(C, pretrained=False).to(DEV), Net(C, pretrained=False).to(DEV)
        opt = fo.FusedSGD(stu, [dict(params=list(stu.pretrained_parameters()), lr=0.01), dict(params=list(stu.new_parameters()), lr=0.1)],
                          momentum=0.9, nesterov=True, weight_decay=5e-4)
        for p in tea.parameters():
            p.requires_grad = False
        ema = optim_weight_ema.EMAWeightOptimizer(tea, stu, 0.99)
        ema.fuse_into(opt)
        stu.train(); tea.train()
        step = CutMixMeanTeacherStep(stu, tea, opt, ema, StepConfig(conf_thresh=0.2, deterministic=True))
        os.environ['CMS_STEP_GRAPH'] = '1'
        out = []
        try:
            for x, y, x0, x1, r in data:
                how = dict(mask=ops.boxmask_rasterize(r, (H, W), True)) if as_mask else dict(ranges=r)
                res = step(x, y, [UnsupBatch(x0, x1_tea=x1, **how)])
                out.append([float(res[k]) for k in ('sup_loss', 'consistency_loss', 'conf_rate')])
            torch.cuda.synchronize()
        finally:
            os.environ.pop('CMS_STEP_GRAPH', None)
            ops.set_deterministic_wgrad(False)
        ents = list(step.__dict__.get('_graphs', {}).values())
        assert sum(1 for v in ents if 'graph' in v) == 1 and not any(v.get('failed') for v in ents)
        grads = {k: p.grad.detach().clone() for k, p in stu.named_parameters() if p.grad is not None}
        return np.array(out), grads, opt.arena.flat.clone()

    la, ga, wa = run(False)
    lb, gb, wb = run(False)
    lm, gm, wm = run(True)
    rel = lambda p, q: float((p - q).abs().max() / (p.abs().max() + 1e-30))
    dl = lambda p, q: float(np.max(np.abs(p - q) / np.abs(p)))
    repeat = np.array_equal(la, lb) and torch.equal(wa, wb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    print('\nU-Net graph replay: ranges {} | mask {}; ranges runs repeat bit for bit: {}; losses mask-ranges {:.2e}, ranges-ranges '
          '{:.2e}; weights {:.2e}, {:.2e}'.format(la[-1], lm[-1], repeat, dl(la, lm), dl(la, lb), rel(wa, wm), rel(wa, wb)))
    assert np.all(np.isfinite(lm)) and set(gm) == set(ga)
    if repeat:
        assert np.array_equal(la, lm) and torch.equal(wa, wm)
        differing = [k for k in ga if not torch.equal(ga[k], gm[k])]
        assert not differing, differing[:8]
    else:
        # the floors and factors of tests/test_gpu_unets.py for runs that do not repeat
        assert dl(la, lm) <= max(2e-2, 4 * dl(la, lb)) and rel(wa, wm) <= max(0.3, 4 * rel(wa, wb))
        assert max(rel(ga[k], gm[k]) for k in ga) <= max(0.3, 4 * max(rel(ga[k], gb[k]) for k in ga))


# ------------------------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize('mask_mode', ['mix', 'zero'])
def test_cowmask_trainer_cli_synthetic_end_to_end(tmp_path, monkeypatch, mask_mode):
    """As tests/test_gpu_executor.py::test_trainer_cli_synthetic_end_to_end: 2 epochs x 2 iterations at a tiny crop."""
    from click.testing import CliRunner
    import train_seg_semisup_cowmask_mt as trainer
    monkeypatch.chdir(tmp_path)
    args = ['--job_desc', 'smoke', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2',
            '--crop_size', '65,65', '--learning_rate', '3e-5', '--lr_sched', 'poly', '--mask_mode', mask_mode,
            '--cow_sigma_range', '2:8', '--conf_thresh', '0.1', '--num_epochs', '2', '--iters_per_epoch', '2',
            '--synthetic_val_batches', '1']
    res = CliRunner().invoke(trainer.experiment, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    log = open(tmp_path / 'results' / 'train_seg_semisup_cowmask_mt' / 'log_smoke.txt').read()
    lines = [l for l in log.splitlines() if l.startswith('Epoch ')]
    assert len(lines) == 2
    pat = re.compile(r'Epoch \d+: took [\d.]+s, TRAIN clf loss=([\d.]+), consistency loss=([\d.]+), conf rate=([\d.]+)%, '
                     r'VAL mIoU=[\d.]+%')
    assert all(pat.match(l) for l in lines), lines
    assert 'Built network' in log and 'Training...' in log and 'Settings:' in log
    assert 'cow_sigma_range=2:8' in log and 'mask_prop_range=0.2:0.8' in log and 'boxmask' not in log
    for l in lines:
        clf, cons, rate = (float(v) for v in pat.match(l).groups())
        assert np.isfinite(clf) and 0 < clf < 10 and np.isfinite(cons) and cons >= 0.0
        assert 0.0 <= rate <= 100.0
