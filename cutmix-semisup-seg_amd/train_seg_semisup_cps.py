"""
Cross pseudo supervision (CPS) with CutMix: two networks of one architecture, initialised differently, each trained with cross
entropy on the other's hard pseudo-labels of a CutMix-ed pair (Chen, Yuan, Zeng, Wang, "Semi-Supervised Semantic Segmentation with
Cross Pseudo Supervision", CVPR 2021), plus the supervised cross entropy on both. The reference has no such program, and the
authors' code was not at hand: the iteration is the paper's as recalled and is this project's definition (cps.py).

The option table is the CutMix trainer's (train_seg_semisup_mask_mt.py) with these changes:
  * removed: `--model`, `--teacher_alpha` (there is no teacher), `--cons_loss_fn`, `--conf_per_pixel` (the loss is cross entropy on
    hard labels, the threshold is per pixel by construction), `--no_fuse_batches`, `--allreduce_dtype` (the step is eager and runs on
    one GPU)
  * `--mask_mode` accepts only `mix`
  * `--cons_weight` defaults to 1.5 (the paper's Pascal VOC value as recalled; not tuned here)
  * `--conf_thresh` defaults to 0.0: CPS has no threshold; the option stays because it costs nothing in the label kernel
The two networks are built one after the other from the same factory, so their random initialisations differ. Network a is the one
that is evaluated every epoch and written as `model.pth` (eval_seg.py scores it as it is); network b is written as `model_2.pth`.
The log has the trainers' `Epoch ...` line and per-class line, then `-- pseudo-label agreement=...%`: the share of valid pixels on
which the two networks' predictions agreed, averaged over the epoch's unsupervised batches. With `--conf_thresh 0` the `conf rate`
column follows the CutMix trainer's rule (the ramp, or 0), as that trainer's does.

The job body is built from trainer_common's pieces, as train_seg_semisup_ict.py's is, not from mask_mt_job: that body builds a
student / teacher pair with an EMA optimiser, one learning-rate schedule, the data-parallel process group and a graph-captured
step, and a hook for each would have cut through most of it. One GPU: WORLD_SIZE > 1 stops before the GPU is touched, as everything
else refusable does.
"""
import click

from . import job_helper, trainer_common as tc
from . import train_seg_semisup_mask_mt as cutmix

REMOVED = ('model', 'teacher_alpha', 'cons_loss_fn', 'conf_per_pixel', 'no_fuse_batches', 'allreduce_dtype')


class _BothOptimizers(object):
    """what lr_schedules needs of an optimiser -- `param_groups` -- over the two networks' optimisers: one schedule moves both"""

    def __init__(self, optim_a, optim_b):
        self.param_groups = list(optim_a.param_groups) + list(optim_b.param_groups)


def build_network(arch, n_classes, dtype, torch_device, opt_type, learning_rate, sgd_momentum, sgd_nesterov, sgd_weight_decay):
    """one network and its optimiser (no EMA partner), as trainer_common.build_networks builds the student"""
    from .architectures import network_architectures
    from . import optim as fused_optim
    net = network_architectures.seg.get(arch)(n_classes, pretrained=False).to(torch_device)
    net.compute_dtype = dtype
    groups = [dict(params=list(net.pretrained_parameters()), lr=learning_rate * 0.1),
              dict(params=list(net.new_parameters()), lr=learning_rate)]
    if opt_type == 'adam':
        return net, fused_optim.FusedAdam(net, groups)
    if opt_type == 'sgd':
        return net, fused_optim.FusedSGD(net, groups, momentum=sgd_momentum, nesterov=sgd_nesterov, weight_decay=sgd_weight_decay)
    raise ValueError('Unknown opt_type {}'.format(opt_type))


@job_helper.job('train_seg_semisup_cps', enumerate_job_names=False)
def train_seg_semisup_cps(submit_config, dataset, arch, freeze_bn,
                          opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                          learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                          bin_fill_holes,
                          crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                          aug_scale_non_uniform, aug_rot_mag,
                          aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                          aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                          mask_mode, mask_prop_range,
                          boxmask_n_boxes, boxmask_fixed_aspect_ratio, boxmask_by_size, boxmask_outside_bounds,
                          boxmask_no_invert,
                          cons_weight, conf_thresh, rampup, unsup_batch_ratio,
                          num_epochs, iters_per_epoch, batch_size,
                          n_sup, n_unsup, n_val, split_seed, split_path, val_seed, save_preds, save_model,
                          num_workers,
                          synthetic=False, synthetic_n_classes=21, synthetic_val_batches=2, compute_dtype='bf16',
                          synthetic_source_size='', deterministic=False):
    settings = locals().copy()
    del settings['submit_config']

    # refused here, before the data set is opened or the GPU is touched
    if mask_mode != 'mix':
        raise ValueError('train_seg_semisup_cps: --mask_mode {} is not built (only mix)'.format(mask_mode))
    source_size = [int(v.strip()) for v in synthetic_source_size.split(',')] if synthetic_source_size else None
    if source_size is not None and len(source_size) != 2:
        raise ValueError('--synthetic_source_size takes h,w')
    if ':' in mask_prop_range:
        lo, hi = mask_prop_range.split(':')
        prop_range = (float(lo.strip()), float(hi.strip()))
    else:
        prop_range = float(mask_prop_range)

    import os
    import numpy as np
    import torch
    from . import lr_schedules, mask_gen, ops
    from .cps import CPSConfig, CrossPseudoStep
    from .step import UnsupBatch

    crop = tc.parse_crop_size(crop_size)
    ds_dict = tc.open_dataset(synthetic, crop, dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path)
    world, _, torch_device = tc.setup_process('train_seg_semisup_cps', data_parallel=False, one_gpu_what='CPS')

    n_classes = int(synthetic_n_classes)
    run = None
    if ds_dict is not None:
        run = tc.DatasetRun(ds_dict, torch_device, batch_size)
        n_classes = run.n_classes
    if bin_fill_holes and n_classes != 2:
        print('Binary hole filling can only be used with binary (2-class) segmentation datasets')
        return
    print('Loaded data')
    dtype = torch.bfloat16 if compute_dtype == 'bf16' else torch.float32
    # one after the other from the same factory: the second draws its initialisation where the first left the generator
    net_a, optim_a = build_network(arch, n_classes, dtype, torch_device, opt_type, learning_rate, sgd_momentum, sgd_nesterov,
                                   sgd_weight_decay)
    net_b, optim_b = build_network(arch, n_classes, dtype, torch_device, opt_type, learning_rate, sgd_momentum, sgd_nesterov,
                                   sgd_weight_decay)
    if freeze_bn and not hasattr(net_a, 'freeze_batchnorm'):
        raise ValueError('Network {} does not support batchnorm freezing'.format(arch))
    print('Built network')
    if deterministic:
        ops.set_deterministic_wgrad(True)

    if iters_per_epoch == -1:
        iters_per_epoch = 1000 if run is None else run.iters_per_epoch(iters_per_epoch)
    schedulers = lr_schedules.make_lr_schedulers(
        optimizer=_BothOptimizers(optim_a, optim_b), total_iters=iters_per_epoch * num_epochs, schedule_type=lr_sched,
        step_epochs=lr_step_epochs, step_gamma=lr_step_gamma, poly_power=lr_poly_power)

    invert = not boxmask_no_invert
    cfg = CPSConfig(cons_weight=cons_weight, conf_thresh=conf_thresh, rampup=rampup, unsup_batch_ratio=unsup_batch_ratio,
                    invert=invert)
    step = CrossPseudoStep(net_a, net_b, optim_a, optim_b, cfg)
    mask_generator = mask_gen.BoxMaskGenerator(prop_range=prop_range, n_boxes=boxmask_n_boxes,
                                               random_aspect_ratio=not boxmask_fixed_aspect_ratio,
                                               prop_by_area=not boxmask_by_size, within_bounds=not boxmask_outside_bounds,
                                               invert=invert)

    H, W = crop
    data = tc.SyntheticData(torch.Generator(device=torch_device).manual_seed(12345), batch_size, crop, n_classes, dtype)
    mask_rng = np.random.RandomState(12345)
    augment = None
    if run is not None:
        # the data set path, as the CutMix trainer's: unseeded draws, two unsupervised streams that share one sampler
        mask_rng = np.random.RandomState()
        augment = run.make_streams(net_a, (H, W), dtype, settings, 2 if cons_weight > 0.0 else 0)
    elif source_size is not None:
        # as in the CutMix trainer: uint8 source images resident in HBM, every batch through the device-side input staging, which
        # hands the unsupervised images over with their validity maps
        from .device_pipeline import DeviceAugmenter
        augment = DeviceAugmenter((H, W), net_a.MEAN, net_a.STD, out_dtype=dtype, rng=np.random.RandomState(54321),
                                  colour_rng=np.random.RandomState(99), **tc.augmenter_options(settings))
        src_pool = torch.randint(0, 256, (4 * batch_size, source_size[0], source_size[1], 3), generator=data.gen, device=torch_device,
                                 dtype=torch.uint8)
        lab_pool = torch.randint(0, n_classes, (4 * batch_size, source_size[0], source_size[1]), generator=data.gen,
                                 device=torch_device).to(torch.uint8)
        pool_pos = [0]

        def staged(with_labels):
            i = pool_pos[0] % 4
            pool_pos[0] += 1
            sl = slice(i * batch_size, (i + 1) * batch_size)
            return augment(src_pool[sl], lab_pool[sl] if with_labels else None)

    tc.print_settings(settings)
    if run is None:
        tc.print_synthetic_dataset(crop, n_classes, world)
    else:
        sup_iter, unsup_iter_0, unsup_iter_1 = (run.print_sizes_and_start(n_sup) + [None, None])[:3]

    def make_batch():
        if run is not None:
            sb = augment.stage(run.pool, next(sup_iter), True)
            batch_x, batch_y = sb['image'], sb['labels']
        elif augment is not None:
            sb = staged(True)
            batch_x, batch_y = sb['image'], sb['labels']
        else:
            batch_x, batch_y = data.images(), data.labels()
        unsup = []
        if cons_weight > 0.0:
            for _r in range(unsup_batch_ratio):
                ranges = ops.ranges_to_device(mask_generator.generate_ranges(batch_size, (H, W), rng=mask_rng), torch_device)
                if augment is not None:
                    if run is not None:
                        u0 = augment.stage(run.pool, next(unsup_iter_0), False)
                        u1 = augment.stage(run.pool, next(unsup_iter_1), False)
                    else:
                        u0, u1 = staged(False), staged(False)
                    unsup.append(UnsupBatch(u0['image'], ranges, um0=u0['mask'], x1_tea=u1['image'], um1=u1['mask'],
                                            x0_stu=u0.get('image_stu'), x1_stu=u1.get('image_stu')))
                    continue
                x0, x1 = data.images(), data.images()
                unsup.append(UnsupBatch(x0, ranges, x1_tea=x1, x0_stu=data.images() if aug_strong_colour else None,
                                        x1_stu=data.images() if aug_strong_colour else None))
        return batch_x, batch_y, unsup

    def agreement_line(_epoch_i):
        agreement = step.pop_agreement()
        print('-- pseudo-label agreement={:.3%}'.format(0.0 if agreement is None else agreement))

    evaluate = run.evaluate_with(net_a, step) if run is not None else data.evaluate_with(net_a, step, synthetic_val_batches)
    # a NaN supervised loss ends the job; a direction without a kept label reports 0, not NaN (cps.py), so the consistency loss is
    # not what tells a dead network
    if not tc.run_epochs(step, make_batch, evaluate, net_a, net_b, net_a, schedulers, num_epochs, iters_per_epoch, freeze_bn,
                         rampup, conf_thresh, n_classes, bin_fill_holes, torch_device, data_parallel=False,
                         nan_checks_consistency=False, polls_step_nan=False, img_per_s_of=(batch_size, world),
                         after_epoch=agreement_line):
        return

    if save_model and submit_config.run_dir is not None:
        from . import checkpoint
        checkpoint.save_model(net_a, os.path.join(submit_config.run_dir, 'model.pth'))
        checkpoint.save_model(net_b, os.path.join(submit_config.run_dir, 'model_2.pth'))

    if run is not None:
        run.finish(net_a, step, save_preds, submit_config, bin_fill_holes)


def _options():
    """the CutMix trainer's table without REMOVED, `--mask_mode` narrowed to mix, and the two defaults that differ"""
    params = []
    for p in cutmix.experiment.params:
        if p.name in REMOVED:
            continue
        if p.name == 'mask_mode':
            p = click.Option(['--mask_mode'], type=click.Choice(['mix']), default='mix')
        elif p.name == 'cons_weight':
            p = click.Option(['--cons_weight'], type=float, default=1.5)
        elif p.name == 'conf_thresh':
            p = click.Option(['--conf_thresh'], type=float, default=0.0)
        params.append(p)
    return params


def _experiment(**params):
    train_seg_semisup_cps.submit(**params)


experiment = click.Command('experiment', params=_options(), callback=_experiment)


if __name__ == '__main__':
    experiment()
