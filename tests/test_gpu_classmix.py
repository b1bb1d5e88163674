"""
GPU: ClassMix masks made on the device (csrc/classmix.hip through ops.classmix_mask and mask_gen.ClassMixGenerator), the teacher
pre-pass and the mask's route through the step, and the ClassMix command.

The oracle is the definition restated in numpy float64 (tests/_classmix_refs.py). The device interpolates in fp32, within 1e-6 of the
restatement on N(0,1) logits (csrc/tta_math.hpp), and no pixel of these inputs has its two best classes closer than 1e-5 (asserted: a
condition on the inputs, not a tolerance): prediction, sets and mask must be EQUAL. Against ops.tta_vote's single-view prediction
the comparison is bit for bit on any input, NaN logits and exact ties included.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import _classmix_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


def _run(ops, logits, keys, size, align, valid=None):
    """-> dict(mask (N,1,H,W) f32, pred (N,H,W) u8, present / chosen: python ints), all on the host"""
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    n = lg.shape[0]
    pred = torch.full((n,) + tuple(size), 255, dtype=torch.uint8, device=DEV)
    sets = torch.full((n, 2), -7, dtype=torch.int64, device=DEV)
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.float32)).to(DEV)
    mask = ops.classmix_mask(lg, keys, size, align_corners=align, valid=v, pred_out=pred, sets_out=sets)
    torch.cuda.synchronize()
    s = sets.cpu().numpy().astype(np.uint64)
    return dict(mask=mask.cpu().numpy(), pred=pred.cpu().numpy(), present=[int(x) for x in s[:, 0]], chosen=[int(x) for x in s[:, 1]])


def _same(got, ref):
    assert np.array_equal(got['pred'], ref['pred'])
    assert got['present'] == ref['present'] and got['chosen'] == ref['chosen']
    assert got['mask'].dtype == np.float32 and np.array_equal(got['mask'], ref['mask'])


def _vote_pred(ops, logits, size, align):
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    return ops.tta_vote([lg], [False], lg.shape[1], size, align_corners=align, want_pred=True)[1].cpu().numpy()


def _popcount(v):
    return bin(v).count('1')


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_equals_the_fp64_restatement_and_the_single_view_vote(ops, name):
    inp, ref = R.case(name)
    print('\ncase', name, R.CASES[name], 'min top-two gap', ref['gap'])
    assert ref['gap'] >= R.MARGIN
    got = _run(ops, inp['logits'], inp['keys'], inp['size'], inp['align'])
    print('differing predictions', int((got['pred'] != ref['pred']).sum()), 'mask pixels', int((got['mask'] != ref['mask']).sum()))
    _same(got, ref)
    assert np.array_equal(got['pred'], _vote_pred(ops, inp['logits'], inp['size'], inp['align']))
    for p, ch in zip(got['present'], got['chosen']):
        assert ch & ~p == 0 and _popcount(ch) == (_popcount(p) + 1) // 2
    if name == 'c64':
        assert got['present'][1] >> 63 == 1 and got['chosen'][1] >> 63 == 1
    if name == 'c1':
        assert got['present'] == [1, 1, 1] and got['chosen'] == [1, 1, 1] and float(got['mask'].min()) == 1.0


@pytest.mark.parametrize('align', [True, False])
def test_prediction_is_the_single_view_votes_on_nan_logits_and_ties(ops, align):
    inp = R.case_inputs('main_ac')
    lg = inp['logits'].copy()
    lg[0, 3, 2, 3] = np.nan
    lg[1, :, 1, :] = np.nan
    lg[2, 5] = lg[2, 9]                                    # exact ties between two classes, wherever they lead
    lg[2, 0, :2] = np.inf
    got = _run(ops, lg, inp['keys'], inp['size'], align)
    want = _vote_pred(ops, lg, inp['size'], align)
    assert np.array_equal(got['pred'], want)
    for i in range(3):
        assert got['present'][i] == R.bits(set(want[i].ravel().tolist()))
    assert not np.any(got['pred'][2] == 9)                 # the first index keeps a tie
    # all-zero logits: every class ties everywhere -> class 0, one class present and chosen, a mask of all ones
    zeros = np.zeros((2, 21, 5, 7), dtype=np.float32)
    got = _run(ops, zeros, inp['keys'][:2], inp['size'], align)
    assert np.array_equal(got['pred'], _vote_pred(ops, zeros, inp['size'], align)) and int(got['pred'].max()) == 0
    assert got['present'] == [1, 1] and got['chosen'] == [1, 1] and float(got['mask'].min()) == 1.0
    # ... and at the identity size
    got = _run(ops, zeros, inp['keys'][:2], (5, 7), align)
    assert got['present'] == [1, 1] and float(got['mask'].min()) == 1.0
    assert np.array_equal(_run(ops, lg, inp['keys'], (5, 7), align)['pred'], _vote_pred(ops, lg, (5, 7), align))


def test_no_workgroup_straddles_two_samples(ops):
    """Sample 0 favours class 0 everywhere, sample 1 class 1: a workgroup that covered the end of one sample and the start of the
    next, or a slot word left over from another sample, would put both classes into one set."""
    for size, lo in (((33, 41), (5, 7)), ((257, 513), (9, 9)), ((17, 19), (17, 19))):
        rng = np.random.RandomState(3)
        lg = rng.standard_normal((2, 4) + lo).astype(np.float32)
        lg[0, 0] += 20.0
        lg[1, 1] += 20.0
        got = _run(ops, lg, rng.random_sample((2, 4)), size, True)
        assert got['present'] == [1, 2] and got['chosen'] == [1, 2], (size, got['present'])
        assert float(got['mask'].min()) == 1.0


@pytest.mark.parametrize('name', ['main_nac', 'slots'])
def test_sample_alone_equals_sample_in_batch(ops, name):
    inp, ref = R.case(name)
    for i in range(inp['logits'].shape[0]):
        one = _run(ops, inp['logits'][i:i + 1], inp['keys'][i:i + 1], inp['size'], inp['align'])
        assert np.array_equal(one['mask'][0], ref['mask'][i]) and np.array_equal(one['pred'][0], ref['pred'][i])
        assert one['present'][0] == ref['present'][i] and one['chosen'][0] == ref['chosen'][i]


def test_dirty_workspace_and_repeated_calls(ops):
    """Through the C ABI with a workspace of the test's own: filled with 0xFF, used for one input, then for another of the same
    shape; the second result is the restatement's, and a repeated call gives the same bits."""
    from cutmix_semisup_seg_amd import _lib
    inp, ref = R.case('slots')
    n, c, h, w = inp['logits'].shape
    H, W = inp['size']
    other = R.case_inputs('slots', seed=5)
    other['logits'][:, 4:] -= 30.0                          # four classes only: present sets that differ from the first call's
    need = int(_lib.fn['cms_classmix_workspace_bytes'](n, H, W))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)

    def call(case):
        lg = torch.from_numpy(case['logits']).to(DEV)
        keys = torch.from_numpy(case['keys']).to(DEV)
        mask = torch.full((n, 1, H, W), -1.0, device=DEV)
        sets = torch.full((2, n), -7, dtype=torch.int64, device=DEV)
        d = _lib.ClassMixDesc()
        d.logits, d.valid, d.keys = lg.data_ptr(), None, keys.data_ptr()
        d.n, d.c, d.h, d.w, d.H, d.W, d.align_corners = n, c, h, w, H, W, 1
        d.mask_out, d.pred_out, d.present_out, d.chosen_out = mask.data_ptr(), None, sets[0].data_ptr(), sets[1].data_ptr()
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
        _lib.check(_lib.fn['cms_classmix'](ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cms_classmix')
        torch.cuda.synchronize()
        return mask, sets

    other_mask, other_sets = call(other)
    assert [_popcount(int(v)) for v in other_sets[0].cpu().numpy().astype(np.uint64)] == [4, 4]
    mask, sets = call(inp)
    assert np.array_equal(mask.cpu().numpy(), ref['mask'])
    assert np.array_equal(sets.cpu().numpy(), np.stack([R.as_int64(ref['present']), R.as_int64(ref['chosen'])]))
    again_mask, again_sets = call(inp)
    assert torch.equal(mask, again_mask) and torch.equal(sets, again_sets)
    back_mask, back_sets = call(other)
    assert torch.equal(back_mask, other_mask) and torch.equal(back_sets, other_sets)
    pred = ws[n * 2048:n * 2048 + n * H * W].cpu().numpy().reshape(n, H, W)      # without pred_out the predictions are in the workspace
    assert int(pred.max()) < 4


def test_equal_keys_are_ordered_by_class_index(ops):
    inp, ref = R.case('main_ac')
    keys = np.zeros_like(inp['keys'])
    keys[1, :] = 0.5
    keys[2, 10:] = -1.0                                     # two groups of equal keys
    want = R.classmix(inp['logits'], keys, inp['size'], True)
    got = _run(ops, inp['logits'], keys, inp['size'], True)
    _same(got, want)
    classes = [c for c in range(21) if got['present'][0] >> c & 1]
    assert got['chosen'][0] == R.bits(classes[:(len(classes) + 1) // 2])


def test_validity_map(ops):
    inp, ref = R.case('main_ac')
    size = inp['size']
    valid = np.ones((3,) + size, dtype=np.float32)
    cls = int(ref['pred'][0, 0, 0])
    valid[0][ref['pred'][0] == cls] = 0.0                   # a class that occurs only under valid == 0
    valid[1, ::2, 1::3] = 0.0
    valid[1, 5, 5] = -2.5                                   # any non-zero value is valid
    valid[2] = 0.0                                          # an all-invalid sample
    want = R.classmix(inp['logits'], inp['keys'], size, True, valid)
    got = _run(ops, inp['logits'], inp['keys'], size, True, valid)
    _same(got, want)
    assert got['present'][0] == ref['present'][0] & ~(1 << cls) and ref['present'][0] >> cls & 1
    assert float(got['mask'][:, 0][valid == 0].max()) == 0.0
    assert got['present'][2] == 0 and got['chosen'][2] == 0 and float(got['mask'][2].max()) == 0.0
    # (N,1,H,W), as the staging hands it over
    lg = torch.from_numpy(inp['logits']).to(DEV)
    m4 = ops.classmix_mask(lg, inp['keys'], size, valid=torch.from_numpy(valid[:, None]).to(DEV))
    assert np.array_equal(m4.cpu().numpy(), want['mask'])


def test_outputs_are_honoured(ops):
    inp, ref = R.case('main_nac')
    lg = torch.from_numpy(inp['logits']).to(DEV)
    n, (H, W) = lg.shape[0], inp['size']
    plain = ops.classmix_mask(lg, inp['keys'], (H, W), align_corners=False)            # nothing optional
    assert tuple(plain.shape) == (n, 1, H, W) and plain.dtype == torch.float32
    assert np.array_equal(plain.cpu().numpy(), ref['mask'])
    out = torch.full((n, 1, H, W), -1.0, device=DEV)
    pred = torch.full((n, H, W), 255, dtype=torch.uint8, device=DEV)
    sets = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    keys_dev = torch.from_numpy(inp['keys']).to(DEV)                                   # keys as a device tensor
    got = ops.classmix_mask(lg, keys_dev, (H, W), align_corners=False, out=out, pred_out=pred, sets_out=sets)
    assert got is out and torch.equal(out, plain)
    assert np.array_equal(pred.cpu().numpy(), ref['pred'])
    assert np.array_equal(sets.cpu().numpy(), np.stack([R.as_int64(ref['present']), R.as_int64(ref['chosen'])], axis=1))
    # a mask that does not start on a 16-byte boundary takes the element-wise path: the same bits
    big = torch.full((n * H * W + 1,), -1.0, device=DEV)
    off = ops.classmix_mask(lg, keys_dev, (H, W), align_corners=False, out=big[1:].view(n, 1, H, W))
    assert torch.equal(off, plain) and float(big[0]) == -1.0
    half = ops.classmix_mask(lg.bfloat16(), keys_dev, (H, W), align_corners=False)     # converted like tta_vote's views
    assert torch.equal(half, ops.classmix_mask(lg.bfloat16().float(), keys_dev, (H, W), align_corners=False))
    for bad in (dict(out=torch.zeros(n, H, W, device=DEV)), dict(pred_out=torch.zeros(n, H, W, device=DEV)),
                dict(sets_out=torch.zeros(n, 2, device=DEV))):
        with pytest.raises(TypeError):
            ops.classmix_mask(lg, keys_dev, (H, W), **bad)
    with pytest.raises(TypeError):
        ops.classmix_mask(lg, keys_dev.float(), (H, W))
    with pytest.raises(ValueError):
        ops.classmix_mask(lg, keys_dev, (H, W), valid=torch.ones(n, H + 1, W, device=DEV))


def test_generator_on_the_device(ops):
    from cutmix_semisup_seg_amd import mask_gen
    inp, _ = R.case('main_ac')
    gen = mask_gen.ClassMixGenerator()
    keys = gen.generate_params(3, 21, rng=np.random.RandomState(77))
    lg = torch.from_numpy(inp['logits']).to(DEV)
    for align in (True, False):
        want = R.classmix(inp['logits'], keys, inp['size'], align)
        assert want['gap'] >= R.MARGIN
        got = gen.torch_masks_from_logits(keys, lg, inp['size'], align)
        assert np.array_equal(got.cpu().numpy(), want['mask'])


# ------------------------------------------------------------------------------------------------------------------ step
def _deeplab_iteration(reference_mask):
    """The teacher's pre-pass and one iteration of the step on the [1,1,1,1]-block DeepLab v2 of tests/test_gpu_cowmask.py
    (He-initialised, frozen BatchNorm, deterministic weight gradients), with the mask the generator makes on the device or with the
    restatement's mask of the same logits -> (scalars, student gradients, facts about the pre-pass)"""
    from cutmix_semisup_seg_amd import ops, optim as fo
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig, UnsupBatch
    from architectures import deeplab2
    import mask_gen
    import optim_weight_ema
    C, N, H, W = 5, 2, 65, 65
    torch.manual_seed(3)
    mk = lambda: deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], C, np.zeros(3), np.ones(3)).to(DEV)
    stu, tea = mk(), mk()
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
    step = CutMixMeanTeacherStep(stu, tea, opt, ema, StepConfig(mask_mode='mix', conf_thresh=0.2, deterministic=True))
    g = torch.Generator(device=DEV).manual_seed(11)
    im = lambda: torch.randn(N, 3, H, W, generator=g, device=DEV).bfloat16()
    y = torch.randint(0, C, (N, 1, H, W), generator=g, device=DEV).to(torch.uint8)
    x, u0, u1 = im(), im(), im()
    # ---- the pre-pass, as train_seg_semisup_mask_mt.mask_mt_job runs it
    gen = mask_gen.ClassMixGenerator()
    keys = gen.generate_params(N, C, rng=np.random.RandomState(5))
    before = {k: v.detach().clone() for k, v in tea.state_dict().items()}
    rng_before = torch.cuda.get_rng_state(DEV).clone()
    with torch.no_grad():
        logits = tea.forward_lowres(u1)
    mask = gen.torch_masks_from_logits(keys, logits, (H, W), step.align_corners)
    torch.cuda.synchronize()
    after = tea.state_dict()
    facts = dict(state_same=set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before),
                 rng_same=torch.equal(rng_before, torch.cuda.get_rng_state(DEV)), n_state=len(before))
    lg = logits.float().cpu().numpy()
    want = R.classmix(lg, keys, (H, W), step.align_corners)
    facts.update(gap=want['gap'], max_abs=float(np.abs(lg).max()), mask_equal=bool(np.array_equal(mask.cpu().numpy(), want['mask'])),
                 share=[float(v) for v in want['mask'].mean(axis=(1, 2, 3))], present=want['present'])
    if reference_mask:
        mask = torch.from_numpy(want['mask']).to(DEV)
    try:
        res = step(x, y, [UnsupBatch(u0, x1_tea=u1, mask=mask)])
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic_wgrad(False)
    grads = {k: p.grad.detach().clone() for k, p in stu.named_parameters() if p.grad is not None}
    return {k: float(v) for k, v in res.items()}, grads, facts


def test_prepass_leaves_the_teacher_alone_and_the_step_takes_the_mask():
    res_d, g_d, facts = _deeplab_iteration(False)
    print('\nClassMix step', res_d, facts)
    assert facts['n_state'] > 10 and facts['state_same'] and facts['rng_same']
    # the condition on the inputs: the fp32 interpolation of logits of this size stays within 4 ulp of their largest magnitude;
    # ten times that, as for the N(0,1) cases
    assert facts['gap'] >= 40 * 2.0 ** -24 * max(1.0, facts['max_abs'])
    assert facts['mask_equal']
    assert set(res_d) >= {'sup_loss', 'consistency_loss', 'conf_rate'}
    assert all(np.isfinite(v) for v in res_d.values()) and res_d['consistency_loss'] > 1e-4
    res_r, g_r, _ = _deeplab_iteration(True)
    assert res_r == res_d
    assert set(g_r) == set(g_d) and len(g_d) > 10
    differing = [k for k in g_d if not torch.equal(g_d[k], g_r[k])]
    assert not differing, differing[:8]


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_classmix_trainer_cli_synthetic_end_to_end(tmp_path, monkeypatch):
    """As tests/test_gpu_cowmask.py::test_cowmask_trainer_cli_synthetic_end_to_end: 2 epochs x 2 iterations at a tiny crop."""
    from click.testing import CliRunner
    import train_seg_semisup_classmix_mt as trainer
    monkeypatch.chdir(tmp_path)
    args = ['--job_desc', 'smoke', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2',
            '--crop_size', '65,65', '--learning_rate', '3e-5', '--lr_sched', 'poly', '--conf_thresh', '0.1', '--num_epochs', '2',
            '--iters_per_epoch', '2', '--synthetic_val_batches', '1']
    res = CliRunner().invoke(trainer.experiment, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    log = open(tmp_path / 'results' / 'train_seg_semisup_classmix_mt' / 'log_smoke.txt').read()
    lines = [l for l in log.splitlines() if l.startswith('Epoch ')]
    assert len(lines) == 2
    pat = re.compile(r'Epoch \d+: took [\d.]+s, TRAIN clf loss=([\d.]+), consistency loss=([\d.]+), conf rate=([\d.]+)%, '
                     r'VAL mIoU=[\d.]+%')
    assert all(pat.match(l) for l in lines), lines
    assert 'Built network' in log and 'Training...' in log and 'Settings:' in log
    assert 'mask_mode=mix' in log and 'boxmask' not in log and 'mask_prop_range' not in log
    for l in lines:
        clf, cons, rate = (float(v) for v in pat.match(l).groups())
        assert np.isfinite(clf) and 0 < clf < 10 and np.isfinite(cons) and cons >= 0.0
        assert 0.0 <= rate <= 100.0


def test_classmix_trainer_cli_with_staged_validity_maps(tmp_path, monkeypatch):
    """As tests/test_gpu_augment.py::test_trainer_cli_with_device_side_staging: the unsupervised images come from the device-side
    staging, rotated, so image 1 arrives with a validity map that has zeros and the mask is made under it."""
    from click.testing import CliRunner
    from cutmix_semisup_seg_amd import ops
    import train_seg_semisup_classmix_mt as trainer
    monkeypatch.chdir(tmp_path)
    seen = []
    real = ops.classmix_mask

    def spy(logits, keys, out_size, align_corners=True, valid=None, **kw):
        mask = real(logits, keys, out_size, align_corners=align_corners, valid=valid, **kw)
        seen.append((valid is not None and bool((valid == 0).any()),
                     valid is None or float((mask * (valid == 0)).max()) == 0.0, tuple(mask.shape)))
        return mask
    monkeypatch.setattr(ops, 'classmix_mask', spy)
    args = ['--job_desc', 'rot', '--synthetic', '--synthetic_source_size', '90,120', '--arch', 'resnet101_deeplab_imagenet',
            '--freeze_bn', '--batch_size', '2', '--crop_size', '65,65', '--aug_rot_mag', '20', '--aug_max_scale', '1.5',
            '--aug_hflip', '--num_epochs', '1', '--iters_per_epoch', '2', '--synthetic_val_batches', '1']
    res = CliRunner().invoke(trainer.experiment, args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert 'Epoch 1' in open(tmp_path / 'results' / 'train_seg_semisup_classmix_mt' / 'log_rot.txt').read()
    assert len(seen) == 2 and all(shape == (2, 1, 65, 65) for _, _, shape in seen)
    assert any(has_zeros for has_zeros, _, _ in seen) and all(zero_under for _, zero_under, _ in seen)
