"""
CPU-only: host-side logic of the drop-in modules (the reference's module names at the repository root) against the
golden vectors generated from the reference: box-mask RNG draws / slicing rules, LR schedules, architecture
registry, DeepLab v2 state-dict layout and parameter groups, CLI surface, job helper, error behaviour.
"""
import hashlib
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch

from conftest import load_golden, load_golden_json

import mask_gen
import lr_schedules
import job_helper
from architectures import network_architectures, deeplab2

_BM = load_golden_json('boxmask_meta')


@pytest.mark.parametrize('case', _BM['cases'], ids=[c['key'] for c in _BM['cases']])
def test_boxmask_generate_params_bit_exact(case):
    g = load_golden('boxmask')
    kw = dict(_BM['flagsets'][case['flagset']])
    pr = kw.pop('prop_range')
    gen = mask_gen.BoxMaskGenerator(tuple(pr) if isinstance(pr, list) else pr, **kw)
    shape = tuple(case['shape'])
    m = gen.generate_params(_BM['n'], shape, rng=np.random.RandomState(case['seed']))
    assert m.dtype == np.float64 and m.shape == (_BM['n'], 1) + shape
    m8 = m.astype(np.uint8)
    assert hashlib.sha256(m8.tobytes()).hexdigest() == case['sha256']
    np.testing.assert_array_equal(m8.sum(axis=3)[:, 0], g[case['key'] + '__rowsum'])
    # the device path carries the same information as int32 ranges
    r = gen.generate_ranges(_BM['n'], shape, rng=np.random.RandomState(case['seed']))
    assert r.dtype == np.int32 and r.shape == (_BM['n'], kw['n_boxes'], 4)
    assert (r[..., 0] <= r[..., 1]).all() and (r[..., 2] <= r[..., 3]).all()
    assert r.min() >= 0 and r[..., 1].max() <= shape[0] and r[..., 3].max() <= shape[1]


def test_boxmask_float_prop_range_and_identity_params():
    gen = mask_gen.BoxMaskGenerator(0.25)
    assert gen.prop_range == (0.25, 0.25)
    t = torch.zeros(2, 1, 8, 8)
    assert gen.torch_masks_from_params(t, (8, 8), 'cpu') is t       # reference: identity (mask_gen.py:119-120)
    with pytest.raises(NotImplementedError):
        mask_gen.MaskGenerator().generate_params(1, (4, 4))


def test_add_mask_params_to_batch_layouts():
    gen = mask_gen.BoxMaskGenerator(0.5, invert=True)
    batch = [dict(image=np.zeros((3, 16, 20), np.float32)) for _ in range(3)]
    out = mask_gen.AddMaskParamsToBatch(gen)(batch)
    assert all(s['mask_params'].shape == (1, 16, 20) and s['mask_params'].dtype == np.float32 for s in out)
    paired = [dict(sample0=dict(image=np.zeros((3, 16, 20), np.float32)), sample1=dict(image=None)) for _ in range(2)]
    out = mask_gen.AddMaskParamsToBatch(gen, as_ranges=True)(paired)
    assert all(s['mask_params'].shape == (1, 4) and s['mask_params'].dtype == np.int32 for s in out)


class _Opt(object):
    def __init__(self, base):
        self.param_groups = [dict(lr=base * 0.1), dict(lr=base)]


def test_lr_schedules_match_reference_sequences():
    g = load_golden('lr')
    base = float(g['base_lr'])
    for sched in ('poly', 'cosine'):
        opt = _Opt(base)
        ep, it = lr_schedules.make_lr_schedulers(opt, 40, sched, '', 0.1, poly_power=0.9)
        assert ep is None and it is not None
        for i in range(40):
            it.step(i)
            np.testing.assert_allclose([gr['lr'] for gr in opt.param_groups], g[sched][i], rtol=1e-12, atol=1e-22)
    opt = _Opt(base)
    ep, it = lr_schedules.make_lr_schedulers(opt, 40, 'stepped', '[3, 6]', 0.1)
    assert it is None and ep is not None
    for e in range(10):
        ep.step(e)
        np.testing.assert_allclose([gr['lr'] for gr in opt.param_groups], g['stepped'][e], rtol=1e-12)
    assert lr_schedules.make_lr_schedulers(_Opt(base), 40, 'none', '', 0.1) == (None, None)
    for bad in (('stepped', ''), ('bogus', '')):       # reference quirk: empty milestones -> "Unknown schedule_type"
        with pytest.raises(ValueError, match='Unknown schedule_type'):
            lr_schedules.make_lr_schedulers(_Opt(base), 40, bad[0], bad[1], 0.1)
    for e, R, v in g['rampup']:
        assert network_architectures.sigmoid_rampup(e, int(R)) == pytest.approx(v, rel=1e-12)


def test_lr_schedules_work_on_torch_optimizers_too():
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([dict(params=[p], lr=0.1)], lr=0.1)
    _, it = lr_schedules.make_lr_schedulers(opt, 10, 'poly', '', 0.1)
    it.step(5)
    assert opt.param_groups[0]['lr'] == pytest.approx(0.1 * 0.5 ** 0.9)


def test_registry_names_and_unavailable_architectures():
    assert sorted(network_architectures.seg.names()) == load_golden_json('registry_names')
    with pytest.raises(NotImplementedError):
        network_architectures.seg.get('resnet101_pspnet_imagenet')(21)
    with pytest.raises(NotImplementedError):
        network_architectures.seg.get('resnet101_deeplabv3_coco')(21)
    with pytest.raises(NotImplementedError, match='cannot be downloaded'):
        network_architectures.seg.get('resnet50unet_imagenet')(2)            # pretrained=True needs the network
    reg = network_architectures.ArchRegistry()

    @reg.register('x')
    def x():
        return 1
    assert reg.get('x') is x and list(reg.names()) == ['x']


def test_unet_encoders_have_torchvisions_published_parameter_counts_and_keys():
    """The U-Net encoders are restated from torchvision 0.5.0's published structure (PARITY UNPINNED, oracle/unets.py):
    what pins them is structural -- parameter counts of resnet50 / resnet101 / densenet161 and torchvision's key names."""
    from architectures import resunet, denseunet
    r50 = resunet.resnet50unet(2, pretrained=False)
    r101 = resunet.resnet101unet(2, pretrained=False)
    d161 = denseunet.densenet161unet(2)
    count = lambda m: sum(p.numel() for p in m.parameters())
    assert count(r50.base_model) == 25557032 and count(r101.base_model) == 44549160 and count(d161.base_model) == 28681000
    ks = list(r50.state_dict().keys())
    assert ks[0] == 'base_model.conv1.weight' and 'base_model.layer4.2.bn3.running_var' in ks and 'base_model.fc.bias' in ks
    assert {'line0_conv.weight', 'line0_conv.bias', 'decoder3.conv.weight', 'decoder0.conv_bn.weight', 'final_dec_conv.weight',
            'final_dec_bn.bias', 'final_clf.bias'} <= set(ks)
    kd = list(d161.state_dict().keys())
    assert kd[0] == 'base_model.features.conv0.weight' and 'base_model.classifier.weight' in kd
    assert 'base_model.features.denseblock3.denselayer36.conv2.weight' in kd and 'base_model.features.transition3.conv.weight' in kd
    assert [(b.x_chn_in, b.chn_out) for b in d161.decoder_blocks] == [(96, 96), (384, 96), (768, 384), (2208, 768)]
    assert d161.line0_conv.in_channels == 2112 and d161.line0_conv.out_channels == 2208
    assert r50.BLOCK_SIZE == (32, 32) and d161.BLOCK_SIZE == (32, 32)
    # parameter groups (resunet.py:97-108, denseunet.py:134-143)
    assert r50.pretrained_parameters() == [] and len(r50.new_parameters()) == len(list(r50.parameters()))
    dimg = denseunet.densenet161unet_imagenet(2, pretrained=False)
    assert len(dimg.pretrained_parameters()) == len(list(dimg.base_model.features.parameters()))
    assert len(dimg.new_parameters()) + len(dimg.pretrained_parameters()) == len(list(dimg.parameters()))
    with pytest.raises(ValueError, match='x_chn_in != skip_chn_in'):
        resunet.DecoderBlock(64, 32, 16)


def test_device_augmenter_draws_parameters_in_the_references_order():
    """device_pipeline.DeviceAugmenter.draw_params against the reference's formulas re-evaluated on the same RandomState
    stream (seg_transforms_cv.py:193-204 Hung scale + position, :122-123 plain crop, :479-480 flips)."""
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    crop, src = (64, 96), (50, 200)              # source shorter than the window in y: padding; wider in x
    aug = DeviceAugmenter(crop, None, None, scale_hung=True, hflip=True, vflip=False, hvflip=False,
                          rng=np.random.RandomState(7))
    got = aug.draw_params(5, src)
    rng = np.random.RandomState(7)
    for i in range(5):
        f = 0.5 + rng.randint(0, 11, size=(1,)) / 10.0
        sc = np.round(np.array(crop) / f).astype(int)
        pad = np.maximum(sc - np.array(src), 0)
        pos = np.round((np.array(src) + pad - sc) * rng.uniform(0.0, 1.0, size=(2,))).astype(int)
        fl = (rng.binomial(1, 0.5, size=(3,)) != 0) & np.array([True, False, False])
        assert tuple(got[i, 2:4]) == tuple(sc) and tuple(got[i, 0:2]) == tuple(pos - pad // 2)
        assert tuple(got[i, 4:7] != 0) == tuple(fl)
        assert got[i, 12] == 0 and tuple(got[i, 7:10]) == (1.0, 1.0, 1.0)          # no colour augmentation asked for
    col = DeviceAugmenter((32, 32), None, None, strong_colour=True, rng=np.random.RandomState(1),
                          colour_rng=np.random.RandomState(2)).draw_params(200, (40, 40))
    assert 0.6 < col[:, 12].mean() < 0.95 and 0.08 < col[:, 11].mean() < 0.35         # p = 0.8 / 0.2
    assert col[:, 7:10].min() >= 0.6 - 1e-6 and col[:, 7:10].max() <= 1.4 + 1e-6 and np.abs(col[:, 10]).max() <= 0.1
    for o in col[:, 13].astype(int):
        assert sorted((o >> s) & 3 for s in (6, 4, 2, 0)) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match='square crop'):
        DeviceAugmenter((32, 48), None, None, hvflip=True)


def test_robust_bce_formula():
    p = torch.tensor([0.2, 0.9])
    t = torch.tensor([0.0, 1.0])
    want = -(t * torch.log(p + 1e-6) + (1 - t) * torch.log(1 - p + 1e-6))
    torch.testing.assert_close(network_architectures.robust_binary_crossentropy(p, t), want)


_DM = load_golden_json('deeplab2_meta')


@pytest.mark.parametrize('tag', ['tiny', 'r101'])
def test_deeplab2_state_dict_and_param_groups(tag):
    from oracle import deeplab2 as odl
    meta = _DM[tag]
    C, layers = meta['num_classes'], meta['layers']
    if tag == 'r101':
        net = network_architectures.seg.get('resnet101_deeplab_imagenet')(C, pretrained=False)
    else:
        net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, layers, C, np.zeros(3), np.ones(3))
    sd = net.state_dict()
    spec = odl.state_spec(C, layers)
    assert list(sd.keys()) == list(spec.keys())
    for k, (shape, dt) in spec.items():
        assert tuple(sd[k].shape) == tuple(shape) and sd[k].dtype == dt
    assert len(sd) == meta['n_state']
    assert sum(p.numel() for p in net.parameters()) == meta['n_params']
    assert sum(p.numel() for p in net.parameters() if p.requires_grad) == meta['n_trainable']
    id2key = {id(p): k for k, p in net.named_parameters()}
    assert [id2key[id(p)] for p in net.pretrained_parameters()] == meta['pretrained_order']
    assert [id2key[id(p)] for p in net.new_parameters()] == meta['new_order']
    assert sorted(net.unused_parameter_keys()) == meta['none_grads_in0']
    assert net.BLOCK_SIZE == (1, 1) and hasattr(net, 'MEAN') and hasattr(net, 'STD')
    if tag == 'r101':
        assert Counter(Counter(meta['pretrained_order']).values()) == {1: 1, 3: 99, 4: 4}
    net.train()
    net.freeze_batchnorm()
    assert all(not m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert net.layer1.training
    # loading closed-form state through the reference-style helper
    deeplab2._load_state_into_model(net, odl.closed_form_state(C, layers))
    torch.testing.assert_close(net.state_dict()['layer1.0.conv1.weight'],
                               odl.closed_form_state(C, layers)['layer1.0.conv1.weight'])


def test_deeplab2_mean_std_of_the_three_factories():
    a = deeplab2.resnet101_deeplab_imagenet(3, pretrained=False)
    b = deeplab2.resnet101_deeplab_coco(3, pretrained=False)
    c = deeplab2.resnet101_deeplab_imagenet_mittal_std(3, pretrained=False)
    np.testing.assert_allclose(a.MEAN, [0.485, 0.456, 0.406])
    np.testing.assert_allclose(a.STD, [0.229, 0.224, 0.225])
    np.testing.assert_allclose(b.MEAN, np.array([122.67891434, 116.66876762, 104.00698793]) / 255.0)
    np.testing.assert_allclose(b.STD, np.ones(3) / 255.0)
    np.testing.assert_allclose(c.MEAN, b.MEAN)


def test_networks_refuse_cpu_inputs():
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 3, np.zeros(3), np.ones(3))
    with pytest.raises(RuntimeError, match='GPU only'):
        net(torch.zeros(1, 3, 33, 33))


def test_cli_surface_matches_reference():
    import train_seg_semisup_mask_mt as trainer
    ref = load_golden_json('cli_options')
    mine = {p.name: p for p in trainer.experiment.params}
    for o in ref:
        assert o['name'] in mine, 'missing option --{}'.format(o['name'])
        p = mine[o['name']]
        assert list(p.opts) == o['opts']
        assert bool(getattr(p, 'is_flag', False)) == o['is_flag']
        assert p.default == o['default'] or str(p.default) == str(o['default']), o['name']
        if o['choices'] is not None:
            assert list(p.type.choices) == o['choices']
    extra = set(mine) - {o['name'] for o in ref}
    assert extra == {'synthetic', 'synthetic_n_classes', 'synthetic_val_batches', 'compute_dtype', 'no_fuse_batches',
                     'synthetic_source_size', 'deterministic', 'allreduce_dtype'}


def test_job_helper_log_layout_and_skip(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    calls = []

    @job_helper.job('myjob', enumerate_job_names=False)
    def fn(submit_config, a):
        calls.append(a)
        print('hello {}'.format(a))
        assert submit_config.run_dir == os.path.join('results', 'myjob', 'd1')

    fn.submit(job_desc='d1', a=3)
    assert calls == [3]
    assert 'hello 3' in open(tmp_path / 'results' / 'myjob' / 'log_d1.txt').read()
    assert (tmp_path / 'results' / 'myjob' / 'd1').is_dir()
    fn.submit(job_desc='d1', a=4)                  # log exists -> skipped
    assert calls == [3]
    assert 'already executed; skipping' in capsys.readouterr().out
    with pytest.raises(ValueError):
        fn.submit(job_desc='d2', a=1, quota_group='x')


def test_trainer_config_errors_before_touching_a_gpu(tmp_path, monkeypatch):
    import train_seg_semisup_mask_mt as trainer
    monkeypatch.chdir(tmp_path)
    defaults = {p.name: p.default for p in trainer.experiment.params}
    defaults['job_desc'] = 'none'
    bad = dict(defaults, mask_mode='bogus')
    with pytest.raises(ValueError, match='Unknown mask_mode'):
        trainer.train_seg_semisup_mask_mt.submit(**bad)


# ------------------------------------------------------------------------------------------------------------------
# host-side decisions of the training step and the engines (no GPU needed: nothing is launched)
def test_step_fuses_batches_only_when_samples_are_independent():
    """Concatenating [x_sup; x_mix] / [x0; x1] is only the same computation when no layer couples the samples of a
    batch: every BatchNorm frozen and no active dropout, in both networks (step.py)."""
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig
    from cutmix_semisup_seg_amd.architectures import deeplab3plus as d3
    v2 = lambda: deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 3, np.zeros(3), np.ones(3))
    stu, tea = v2(), v2()
    step = CutMixMeanTeacherStep(stu, tea, None, None, StepConfig())
    stu.train(); tea.train()
    assert not step._samples_independent()                 # batch-statistics BatchNorm
    stu.freeze_batchnorm()
    assert not step._samples_independent()                 # ... still in the teacher
    tea.freeze_batchnorm()
    assert step._samples_independent()
    # DeepLab v3+: freeze_batchnorm() covers the backbone only, the head keeps batch statistics and dropout
    w = d3.DeepLabv3Wrapper(d3._deeplabv3plus(3, 8, (1, 1, 1, 1)))
    w.train(); w.freeze_batchnorm()
    step3 = CutMixMeanTeacherStep(w, w, None, None, StepConfig())
    assert not step3._samples_independent()
    w.eval()
    assert step3._samples_independent()


def test_step_groups_batches_under_batch_statistics_only_where_the_kernels_keep_groups_apart():
    """Batch-statistics BatchNorm: the passes may still travel as [sup; mixed] / [x0; x1] when both networks normalise SAMPLE
    GROUPS apart (step._sample_groups): DeepLab v2 on the executor and DeepLab v3+, equal batch sizes, separate student /
    teacher objects, one process -- decided on the host, checked here without a GPU."""
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig, UnsupBatch
    from cutmix_semisup_seg_amd.architectures import deeplab3plus as d3
    v2 = lambda: deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 3, np.zeros(3), np.ones(3))
    stu, tea = v2(), v2()
    stu.train(); tea.train()
    step = CutMixMeanTeacherStep(stu, tea, None, None, StepConfig())
    ub = lambda n: UnsupBatch(torch.zeros(n, 3, 9, 9), None, x1_tea=torch.zeros(n, 3, 9, 9))
    assert stu.supports_sample_groups() and stu.sample_groups() == 1
    assert step._sample_groups(4, [ub(4)], True) == (2, 2)
    assert step._sample_groups(4, [ub(4), ub(4)], True) == (3, 4)
    assert step._sample_groups(4, [], False) == (1, 0)
    assert step._sample_groups(4, [ub(3)], True) is None                    # unequal group sizes
    step.cfg.mix = False
    assert step._sample_groups(4, [ub(4)], True) == (2, 1)                  # cut mode: one teacher pass
    step.cfg.mix = True
    tea.batchstat_executor = False                                          # teacher on the layer engine: no grouped kernels there
    assert step._sample_groups(4, [ub(4)], True) is None
    tea.batchstat_executor = True
    pi = CutMixMeanTeacherStep(stu, stu, None, None, StepConfig())          # Pi model: ONE set of running statistics
    assert pi._sample_groups(4, [ub(4)], True) is None
    stu.freeze_batchnorm()
    assert not stu.supports_sample_groups()                                 # frozen statistics: nothing to group (plain fusion)
    stu.set_sample_groups(3)
    assert stu.sample_groups() == 3
    from cutmix_semisup_seg_amd import checkpoint
    assert '_bn_groups' not in checkpoint.export_module(stu).__dict__       # runtime state stays out of checkpoints
    stu.set_sample_groups(1)
    w, wt = (d3.DeepLabv3Wrapper(d3._deeplabv3plus(3, 8, (1, 1, 1, 1))) for _ in range(2))
    for n in (w, wt):
        n.train(); n.freeze_batchnorm()
    s3 = CutMixMeanTeacherStep(w, wt, None, None, StepConfig())
    assert w.supports_sample_groups() and s3._sample_groups(2, [ub(2)], True) == (2, 2)      # head BatchNorms, dropout active
    w.eval()
    assert not w.supports_sample_groups()


def test_which_convolutions_of_the_v3plus_head_are_routed_to_the_mfma_kernels():
    from cutmix_semisup_seg_amd.backbone_hip import hip_conv2d_eligible
    from cutmix_semisup_seg_amd.architectures import deeplab3plus as d3

    class FakeCuda(object):                      # shape / dtype / device facts only -- nothing is computed
        def __init__(self, shape, dtype=torch.bfloat16, cuda=True):
            self.shape, self.dtype, self.is_cuda = shape, dtype, cuda

    from cutmix_semisup_seg_amd import backbone_hip
    head = d3.DeepLabHeadV3Plus(2048, 256, 21)
    x65 = lambda c: FakeCuda((10, c, 65, 65))
    stem = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    grouped = torch.nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False)
    # 'auto' sends EVERY convolution the general hand-written path can express to it -- the pooled branch's 1 x 1-map GEMM (the
    # last library kernel of the cfg 4 step until round 5), strided layers, the 7 x 7 stem included; what it cannot express raises
    # in the engine (round 6: there is no library fallback, and no CMS_AUTO_LIBRARY switch any more)
    assert not hasattr(backbone_hip, '_auto_keeps_library')
    assert all(hip_conv2d_eligible(x65(2048), head.aspp.convs[i][0]) for i in range(4))
    assert hip_conv2d_eligible(x65(1280), head.aspp.project[0])
    assert hip_conv2d_eligible(FakeCuda((10, 304, 129, 129)), head.classifier[0])            # padded to 320 channels
    assert hip_conv2d_eligible(FakeCuda((10, 256, 129, 129)), head.project[0])               # 48 outputs, padded to 64
    assert hip_conv2d_eligible(FakeCuda((10, 2048, 1, 1)), head.aspp.convs[4][1])
    assert hip_conv2d_eligible(FakeCuda((10, 3, 513, 513)), stem)
    assert hip_conv2d_eligible(FakeCuda((10, 2048, 65, 65), torch.float32), head.aspp.convs[1][0], torch.float32)
    assert not hip_conv2d_eligible(FakeCuda((10, 64, 65, 65)), grouped)                  # no hand-written grouped convolution
    assert not hip_conv2d_eligible(FakeCuda((10, 2048, 65, 65), torch.float32), head.aspp.convs[1][0])      # engine dtype differs
    assert not hip_conv2d_eligible(FakeCuda((10, 2048, 65, 65), cuda=False), head.aspp.convs[1][0])


def test_v3plus_engine_selection_flags():
    from cutmix_semisup_seg_amd.architectures import deeplab3plus as d3
    w = d3.DeepLabv3Wrapper(d3._deeplabv3plus(3, 8, (1, 1, 1, 1)))
    w.train()
    assert not w._use_hip_backbone()                       # backbone BatchNorm on batch statistics
    w.freeze_batchnorm()
    assert w._use_hip_backbone()                           # training passes included
    w.engine_kind = 'hip_nograd'
    assert not w._use_hip_backbone()
    with torch.no_grad():
        assert w._use_hip_backbone()
    w.engine = object()                                    # an explicit engine object (the tests' library engine) switches it off
    assert not w._use_hip_backbone()
    w.engine = None
    w.engine_kind, w.compute_dtype = 'auto', torch.float32
    assert w._use_hip_backbone()                           # round 5: 'auto' in fp32 is the hand-written fp32 configuration too
    w.engine_kind = 'hip_nograd'
    assert not w._use_hip_backbone()                       # (fp32 + 'hip_nograd': not a configuration of the executor)


# ------------------------------------------------------------------------------------------------------------------
# VAT trainer
def test_vat_cli_surface_matches_reference():
    import train_seg_semisup_vat_mt as trainer
    ref = load_golden_json('cli_options_vat')
    mine = {p.name: p for p in trainer.experiment.params}
    for o in ref:
        assert o['name'] in mine, 'missing option --{}'.format(o['name'])
        p = mine[o['name']]
        assert list(p.opts) == o['opts']
        assert bool(getattr(p, 'is_flag', False)) == o['is_flag']
        assert p.default == o['default'] or str(p.default) == str(o['default']), o['name']
        if o['choices'] is not None:
            assert list(p.type.choices) == o['choices']
    assert set(mine) - {o['name'] for o in ref} == {'synthetic', 'synthetic_n_classes', 'synthetic_val_batches',
                                                     'compute_dtype'}


def test_vat_oracle_math_on_a_linear_network():
    """oracle/vat.py on a network whose Jacobian is known: logits = conv(x, W). With the 'logits_var' distance and
    x_hat == x the power-iteration step is d/d eps |W eps|^2 = 2 W^T W eps, i.e. the normalised W^T W eps0."""
    from oracle import vat as ov
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    # float64: with x_hat == x the step differentiates |f(x + eps) - f(x)|^2 at eps ~ 1e-9 per pixel, which float32
    # (the reference's precision) resolves to mostly zeros -- in unpaired mode the reference's direction is largely
    # rounding noise; the identity itself is exact
    w = torch.randn(5, 3, 3, 3, generator=g, dtype=torch.float64)
    net = lambda x: F.conv2d(x, w, padding=1)
    x = torch.randn(2, 3, 9, 11, generator=g, dtype=torch.float64)
    eps0 = ov.normalize_eps(torch.randn(x.shape, generator=g, dtype=torch.float64)) * ov.noise_scale(x.shape)
    assert ov.noise_scale(x.shape) == pytest.approx(1e-6 * 9 * 11 / 1000)
    d, y = ov.vat_direction(net, x, x, eps0, 'logits_var')
    want = ov.normalize_eps(F.conv_transpose2d(F.conv2d(eps0, w, padding=1), w, padding=1))
    assert float((d - want).abs().max()) <= 1e-6 * float(want.abs().max())
    torch.testing.assert_close(d.reshape(2, -1).norm(dim=1), torch.ones(2, dtype=torch.float64), rtol=1e-5, atol=1e-5)   # (the + 1e-12)
    torch.testing.assert_close(y, net(x))
    # radius: global (:298-299) and adaptive (:277-296)
    assert ov.vat_radius_of(x, 0.5, False) == pytest.approx(0.5 * (3 * 9 * 11) ** 0.5)
    r = ov.vat_radius_of(x, 0.5, True)
    man = [0.25 * float(((x[i, :, 2:, :] - x[i, :, :-2, :]) ** 2).sum() + ((x[i, :, :, 2:] - x[i, :, :, :-2]) ** 2).sum()) ** 0.5
           for i in range(2)]
    np.testing.assert_allclose(r.reshape(-1).numpy(), man, rtol=1e-5)
    p, _ = ov.vat_perturbation(net, x, x, eps0, 0.5, False, 'logits_var')
    torch.testing.assert_close(p.reshape(2, -1).norm(dim=1), torch.full((2,), 0.5 * (3 * 9 * 11) ** 0.5, dtype=torch.float64),
                               rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        ov.direction_loss(y, y, 'logits_smoothl1')


def test_vat_host_helpers_match_the_oracle():
    from oracle import vat as ov
    from cutmix_semisup_seg_amd import vat
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 3, 10, 12, generator=g)
    torch.testing.assert_close(vat.normalize_eps(x), ov.normalize_eps(x))
    torch.testing.assert_close(vat.vat_radius_of(x, 0.7, True), ov.vat_radius_of(x, 0.7, True))
    assert vat.vat_radius_of(x, 0.7, False) == ov.vat_radius_of(x, 0.7, False)
    n = vat.normalized_noise_like(x, 2.5, generator=torch.Generator().manual_seed(1))
    torch.testing.assert_close(n.reshape(3, -1).norm(dim=1), torch.full((3,), 2.5))
    with pytest.raises(ValueError):
        vat.VATConfig(cons_loss_fn='logits_smoothl1')


def test_gaussian_kernels_match_the_reference_vectors():
    """mask_gen.gaussian_kernels (reference mask_gen.py:26-43): rows of normalised 1-D Gaussians, width set by the largest
    sigma -- against tests/golden/gaussian_kernels.npz, written by the reference's own function."""
    import os
    import numpy as np
    import mask_gen
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gaussian_kernels.npz'))
    np.testing.assert_allclose(mask_gen.gaussian_kernels(g['sigma']), g['auto'], rtol=1e-14, atol=0)
    np.testing.assert_allclose(mask_gen.gaussian_kernels(g['sigma'], max_sigma=6.0, truncate=3.0), g['wide'], rtol=1e-14, atol=0)
    assert g['auto'].shape == (4, 33) and g['wide'].shape == (4, 37)


def test_product_package_has_no_library_convolution_or_batchnorm_call():
    """the MIOpen comparison engine lives under tests/ (tests/_library_engine.py); the product package holds no
    `F.conv2d` / `F.batch_norm` call, no guarded library branch and no environment switch that enables one. `engine_kind = 'torch'`
    (how rounds 2-5 selected the library engine) now raises and says where the engine went."""
    import re
    from architectures import deeplab2
    from cutmix_semisup_seg_amd.architectures import deeplab3plus as d3
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cutmix-semisup-seg_amd')
    bad = re.compile(r'F\.conv2d|F\.batch_norm|torch\.conv2d|conv_transpose2d|cudnn|miopen_|CMS_LIBRARY_ENGINE|CMS_AUTO_LIBRARY')
    hits = []
    for root, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                for i, line in enumerate(open(os.path.join(root, f)), 1):
                    if bad.search(line):
                        hits.append('{}:{}: {}'.format(os.path.relpath(os.path.join(root, f), pkg), i, line.strip()))
    assert not hits, hits
    assert not hasattr(deeplab2, 'TorchEngine') and not hasattr(deeplab2, 'enable_library_engine')
    eng = deeplab2.LayerEngine(torch.float32)
    with pytest.raises(NotImplementedError, match='HipConvEngine'):
        eng.conv2d(torch.zeros(1, 3, 8, 8), torch.nn.Conv2d(3, 8, 3))
    bn = torch.nn.BatchNorm2d(8).train()
    with pytest.raises(RuntimeError, match='no library fallback'):            # CPU tensor: no csrc/bn.hip, and nothing else
        eng.bn_act(torch.zeros(2, 8, 4, 4), bn, relu=True)

    class FakeCuda(object):
        is_cuda = True
    w = d3.DeepLabv3Wrapper(d3._deeplabv3plus(3, 8, (1, 1, 1, 1)))
    w.engine_kind = 'torch'
    with pytest.raises(RuntimeError, match='tests/_library_engine.py'):
        w._engine(FakeCuda())
    # and the comparison engine itself works where the tests use it on the CPU (fp32 wiring check of the v3+ module tree)
    from _library_engine import LibraryEngine
    lib = LibraryEngine(torch.float32)
    y = lib.conv_bn_act(torch.randn(2, 3, 8, 8), torch.nn.Conv2d(3, 8, 3, padding=1, bias=False), bn, relu=True)
    assert tuple(y.shape) == (2, 8, 8, 8) and float(y.min()) >= 0.0 and int(bn.num_batches_tracked) == 1


def test_bench_final_line_is_compact_and_strict_json():
    """the driver keeps a bounded tail of stdout, a 33 KB line lost its head and nothing parsed. The LAST stdout line of
    bench.py is built by `bench.compact_line` from the complete result object: scalars and short objects only, <= 4096 bytes,
    strict JSON (no NaN / Infinity), carrying `roofline` and `cpu_baseline`."""
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench
    long_name = 'void cms::conv_igemm_kernel<2, 2, 2, 2, true, 1, 64, false, 0, true, false>(cms::ConvArgs)' * 3
    per_wl = {'workload': 'pascal', 'value': 626.7657951795444, 'config': {'x': list(range(500))},
              'roofline': {'by_kernel': {long_name + str(i): {'a': 1.0} for i in range(40)}}}
    full = {
        'metric': 'train images/sec (student+teacher step)', 'value': 626.7657951795444, 'unit': 'images/sec', 'n_gpus': 1,
        'rccl_world_size': 1, 'steps': 20, 'warmup': 5, 'ms_per_step': 15.954922998207621, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': 'bf16', 'data': 'synthetic ' * 40,
        'config': {'workload': 'deeplab2-resnet101 cutmix mean-teacher step, 10x3x321x321, 21 classes (BASELINE configs[1])',
                   'per_gpu_batch': 10, 'global_batch': 10, 'crop': [321, 321], 'parallelism': 'dp1',
                   'stream_probe': [[0, 0.09, [[0] * 7] * 7, [1, 2, 3]]] * 4, 'parity_config': 'p' * 400,
                   'last_losses': {'sup_loss': float('nan')}, 'value_512x1024': 132.5, 'ms_per_step_512x1024': 30.17,
                   'also_v3plus_513x513_img_s': 150.8, 'also_no_freeze_bn_321x321_img_s': 342.6,
                   'host_enqueue_ms_per_step': float('inf')},
        'roofline': {'bound': 'mfma', 'kernel': 'k' * 300, 'achieved': 381.6, 'peak': 2500.0, 'unit': 'TFLOP/s', 'frac': 0.1526,
                     'traffic': 112636718.7, 'avg_launch_ms': 0.0737, 'algorithmic_flops_per_launch': 28153523563.35,
                     'algorithmic_bytes_per_launch': 95933171.2, 'mixed_frac': 0.416, 'step_mfma_frac': 0.295,
                     'isolated_frac': float('nan'), 'hbm_group_frac': 0.146, 'mixed_frac_512x1024': 0.439,
                     'mixed': {'frac': 0.416, 'basis': 'b' * 200}, 'by_kernel': per_wl['roofline']['by_kernel'],
                     'traffic_by_kernel': {long_name: {'ratio': 1.29, 'pmc_bytes_per_launch': 1.0},
                                           'cms::w8::wgrad8_kernel(cms::w8::Args)': {'ratio': 2.06},
                                           'void cms::c8::conv8_kernel<false, false>(cms::c8::Args)': {'ratio': 1.3}},
                     'traffic_source': 's' * 300, 'sampling': 'every 5th launch'},
        'roofline_hbm': {'bound': 'hbm', 'peak': 8000.0, 'unit': 'GB/s', 'achieved': 1169.0, 'frac': 0.146, 'basis': 'b' * 300,
                         'ms_per_step': 0.867, 'parts': {str(i): {'ms_per_step': 0.1} for i in range(6)}, 'traffic': None},
        'cpu_baseline': {'value': 1.0156, 'unit': 'images/sec', 'cores': 32, 'kind': 'port', 'sample': 'oracle/step.py ' * 30},
        'value_321x321': 626.7657951795444, 'value_512x1024': 132.5, 'configs': [per_wl] * 2, 'also': [per_wl] * 2,
        'detail': 'bench_detail.json'}
    assert len(json.dumps(full)) > 32768                         # the kind of object that broke round 5's record
    line = bench.compact_line(full)
    assert '\n' not in line and len(line) <= 4096 == bench.LINE_LIMIT

    def strict(tok):
        raise AssertionError('non-standard JSON constant ' + tok)
    d = json.loads(line, parse_constant=strict)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['data'] == 'synthetic' and d['config']['workload'].startswith('deeplab2-resnet101')
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'mixed_frac', 'step_mfma_frac', 'hbm_group_frac',
              'mixed_frac_512x1024', 'traffic_ratio_wgrad8', 'traffic_ratio_conv8', 'traffic_ratio'):
        assert k in d['roofline'], k
    assert len(d['roofline']['kernel']) <= 80 and d['roofline']['isolated_frac'] is None
    assert d['config']['value_512x1024'] == 132.5 and d['config']['also_v3plus_513x513_img_s'] == 150.8
    assert set(d['cpu_baseline']) == {'value', 'unit', 'cores', 'kind', 'sample'}
    assert not any(isinstance(v, (dict, list)) for o in (d['config'], d['roofline'], d['roofline_hbm'], d['cpu_baseline'])
                   for v in o.values())
    # the committed complete object of round 5 (33 KB, the one the driver could not keep) through the same function
    r5 = os.path.join(repo, 'profiles', 'r05zz_bench_default.json')
    if os.path.exists(r5):
        l5 = bench.compact_line(json.load(open(r5)))
        assert len(l5) <= 4096 and json.loads(l5, parse_constant=strict)['value'] == pytest.approx(626.766, rel=1e-5)


def test_bench_plain_run_times_the_headline_only_and_full_keeps_the_rest():
    """A plain `bench.py --gpus 1 --steps K --warmup W` times the 321 x 321 headline and nothing else; --full restores what the
    default run did before (both shapes, the `also` runs, event brackets, extra steps, CPU baseline, PMC passes); explicit
    options still win."""
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench
    plain = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (plain.steps, plain.warmup, plain.full, plain.dump_outputs) == (7, 2, False, '')
    assert plain.workload == 'pascal' and plain.traffic == 'omit'
    assert plain.no_cpu_baseline and plain.no_also and plain.timed_only and plain.no_roofline_events
    full = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2', '--full'])
    assert full.workload == 'both' and full.traffic == 'measure'
    assert not (full.no_cpu_baseline or full.no_also or full.timed_only or full.no_roofline_events)
    mixed = bench.parse_args(['--full', '--workload', 'pascal', '--traffic', 'omit', '--no_cpu_baseline', '--dump-outputs', 'd'])
    assert mixed.workload == 'pascal' and mixed.traffic == 'omit' and mixed.no_cpu_baseline and not mixed.no_also
    assert mixed.dump_outputs == 'd'


def test_bench_dump_outputs_are_float_npy_files_within_the_limit(tmp_path):
    """--dump-outputs: the step's returned scalars and a seeded sample of both networks' parameters, float32, the same sample
    every time; anything but float32 / float64 or more than the byte limit is refused."""
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench
    torch.manual_seed(0)
    stu, tea = torch.nn.Linear(300, 200), torch.nn.Linear(300, 200)
    res = dict(sup_loss=torch.tensor(1.25), consistency_loss=torch.tensor(0.5), conf_rate=None)
    a = bench.dump_arrays(res, stu, tea, n=1000)
    b = bench.dump_arrays(res, stu, tea, n=1000)
    assert sorted(a) == ['consistency_loss', 'student_params_sample', 'sup_loss', 'teacher_params_sample']
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    flat = torch.cat([p.detach().reshape(-1) for p in stu.parameters()]).numpy()
    assert a['student_params_sample'].shape == (1000,) and np.isin(a['student_params_sample'], flat).all()
    assert float(a['sup_loss'][0]) == 1.25
    names = bench.write_outputs(str(tmp_path / 'out'), a)
    assert sorted(names) == sorted(k + '.npy' for k in a)
    for k in a:
        assert np.array_equal(np.load(str(tmp_path / 'out' / (k + '.npy'))), a[k])
    with pytest.raises(TypeError):
        bench.write_outputs(str(tmp_path / 'bad'), {'i': np.zeros(3, np.int64)})
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / 'big'), {'x': np.zeros(1000, np.float32)}, limit=100)
    assert bench.DUMP_SAMPLE * 4 * 2 < bench.DUMP_LIMIT


def test_hipgraph_replay_is_chosen_for_layer_engine_networks_only(monkeypatch):
    """(round 6) The gradient passes are captured into a hipGraph and replayed where every launch goes through Python (the U-Nets:
    host-bound), not for the DeepLab networks whose passes are recorded programs; one process only; the environment switches force
    it either way (vat.VATMeanTeacherStep.use_graph, step.CutMixMeanTeacherStep._graph_wanted)."""
    from cutmix_semisup_seg_amd.step import CutMixMeanTeacherStep, StepConfig
    from cutmix_semisup_seg_amd import vat
    from cutmix_semisup_seg_amd.architectures import deeplab3plus as d3, network_architectures
    monkeypatch.delenv('CMS_STEP_GRAPH', raising=False)
    monkeypatch.delenv('CMS_VAT_GRAPH', raising=False)
    v2 = lambda: deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 3, np.zeros(3), np.ones(3))
    v3 = lambda: d3.DeepLabv3Wrapper(d3._deeplabv3plus(3, 8, (1, 1, 1, 1)))
    unet = lambda: network_architectures.seg.get('resnet50unet_imagenet')(2, pretrained=False)
    for mk, want in ((v2, False), (v3, False), (unet, True)):
        stu, tea = mk(), mk()
        assert CutMixMeanTeacherStep(stu, tea, None, None, StepConfig())._graph_wanted() is want
        assert vat.VATMeanTeacherStep(stu, tea, None, None, vat.VATConfig()).use_graph is want
    stu, tea = unet(), unet()
    mixed = CutMixMeanTeacherStep(stu, v2(), None, None, StepConfig())          # one of the two on an executor: launch by launch
    assert not mixed._graph_wanted()
    step = CutMixMeanTeacherStep(stu, tea, None, None, StepConfig())
    step.world = 2                                                              # data parallel: SyncBN exchanges are host operations
    assert not step._graph_wanted()
    step.world = 1
    monkeypatch.setenv('CMS_STEP_GRAPH', '0')
    assert not step._graph_wanted()
    monkeypatch.setenv('CMS_STEP_GRAPH', '1')
    assert CutMixMeanTeacherStep(v2(), v2(), None, None, StepConfig())._graph_wanted()
    monkeypatch.setenv('CMS_VAT_GRAPH', '0')
    assert not vat.VATMeanTeacherStep(stu, tea, None, None, vat.VATConfig()).use_graph
    monkeypatch.setenv('CMS_VAT_GRAPH', '1')
    assert vat.VATMeanTeacherStep(v2(), v2(), None, None, vat.VATConfig()).use_graph
