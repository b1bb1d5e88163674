"""
Mirror of the reference's train_seg_semisup_mask_mt.py: CutMix / Cutout mean-teacher (or Pi-model) trainer with the
same 56 command-line options (names and defaults, train_seg_semisup_mask_mt.py:581-638), the same job/log layout
(job_helper) and the same per-epoch log lines (:521-530, :576-577), driving the MI355X step (step.py).

Differences, all additive:
  * `--synthetic` (plus `--synthetic_n_classes`, `--synthetic_val_batches`) trains on synthetic tensors of the crop
    shape. Synthetic runs use `pretrained=False`.
  * without `--synthetic`, `--dataset pascal` / `pascal_aug` / `camvid` / `cityscapes` / `isic2017` train on the data set that
    `./semantic_segmentation.cfg` locates (a directory tree for Pascal VOC, one ZIP file each for the others)
    (settings.py, datapipe/; trainer_common.open_dataset / DatasetRun, shared by the four trainers): the reference's splits and
    index streams on the host, every image decoded once into an HBM-resident pool (resident_pool.py), training crops and padded evaluation batches gathered on the device
    (device_pipeline.DeviceAugmenter.stage / stage_eval, csrc/stage.hip); VAL mIoU every epoch, FINAL TEST with
    `--n_val`. One GPU, a `--crop_size` is required, weights from the package's initialisation (no pretrained
    files here). A data set whose location is not configured stops with a clear message. On this path `--synthetic_source_size`,
    `--synthetic_n_classes` and `--synthetic_val_batches` have no effect (sizes, classes and the validation set are the
    data set's), `--num_workers` is accepted and unused, and the crop / flip / colour / mask draws are unseeded numpy
    streams as in the reference (the index streams follow `torch.manual_seed`).
  * `--compute_dtype {bf16,fp32}` and `--no_fuse_batches`.
  * one process per GPU under torchrun (RANK / LOCAL_RANK / WORLD_SIZE); the reference is single-GPU (`cuda:0`, :58).
  * losses are accumulated on the device and read back once per epoch instead of three host syncs per iteration;
    the NaN bail (:469-472) fires one iteration late.
  * the job body (`mask_mt_job`) is shared with train_seg_semisup_cowmask_mt.py and train_seg_semisup_classmix_mt.py, which differ in
    their mask generators and in the options those read; this command's option table, settings line and log are what they were.
"""
import click

from . import job_helper, trainer_common as tc


@job_helper.job('train_seg_semisup_mask_mt', enumerate_job_names=False)
def train_seg_semisup_mask_mt(submit_config, dataset, model, arch, freeze_bn,
                              opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                              learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                              teacher_alpha, bin_fill_holes,
                              crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                              aug_scale_non_uniform, aug_rot_mag,
                              aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                              aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                              mask_mode, mask_prop_range,
                              boxmask_n_boxes, boxmask_fixed_aspect_ratio, boxmask_by_size, boxmask_outside_bounds,
                              boxmask_no_invert,
                              cons_loss_fn, cons_weight, conf_thresh, conf_per_pixel, rampup, unsup_batch_ratio,
                              num_epochs, iters_per_epoch, batch_size,
                              n_sup, n_unsup, n_val, split_seed, split_path, val_seed, save_preds, save_model,
                              num_workers,
                              synthetic=False, synthetic_n_classes=21, synthetic_val_batches=2, compute_dtype='bf16',
                              no_fuse_batches=False, synthetic_source_size='', deterministic=False,
                              allreduce_dtype='fp32'):
    settings = locals().copy()
    del settings['submit_config']

    common = {k: v for k, v in settings.items() if not k.startswith('boxmask_')}

    def box_masks(prop_range):
        from . import mask_gen
        return mask_gen.BoxMaskGenerator(prop_range=prop_range, n_boxes=boxmask_n_boxes,
                                         random_aspect_ratio=not boxmask_fixed_aspect_ratio, prop_by_area=not boxmask_by_size,
                                         within_bounds=not boxmask_outside_bounds, invert=not boxmask_no_invert)

    # inherited, not chosen: only a NaN SUPERVISED loss ends the job, and the step's NaN flag is polled every iteration (the other
    # three trainers check both losses and do not poll)
    return mask_mt_job('train_seg_semisup_mask_mt', submit_config, settings, box_masks, invert=not boxmask_no_invert,
                       nan_checks_consistency=False, polls_step_nan=True, **common)


def teacher_prepass_moves(net, freeze_bn):
    """None when a forward pass of `net` in training mode (after freeze_batchnorm() with `freeze_bn`) changes nothing but its
    output, else why not: a BatchNorm on batch statistics moves its running statistics, an active Dropout draws from the
    generator. Looks at the modules only: works on a network that has never left the host."""
    was_training = net.training
    modes = [(m, m.training) for m in net.modules()]
    try:
        net.train()
        if freeze_bn:
            net.freeze_batchnorm()
        # by name, as architectures/util.freeze_bn_module finds its layers
        bn = [k for k, m in net.named_modules() if 'BatchNorm' in type(m).__name__ and m.training
              and getattr(m, 'track_running_stats', True)]
        drop = [k for k, m in net.named_modules() if 'Dropout' in type(m).__name__ and m.training and getattr(m, 'p', 1.0) > 0]
    finally:
        for m, mode in modes:
            m.training = mode
        assert net.training == was_training
    if bn and not freeze_bn:
        return ('the mask is made from a teacher pass before the step, which must not move the teacher: {} BatchNorm layers would '
                'update their running statistics; run with --freeze_bn'.format(len(bn)))
    if bn or drop:
        return ('the mask is made from a teacher pass before the step, which must not move the teacher: this architecture keeps {} '
                'BatchNorm layers on batch statistics and {} active Dropout layers even with --freeze_bn (first: {}); it is not '
                'supported by this command'.format(len(bn), len(drop), (bn + drop)[0]))
    return None


def mask_mt_job(job_name, submit_config, settings, make_mask_generator, invert, nan_checks_consistency, polls_step_nan,
                dataset, model, arch, freeze_bn,
                opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                teacher_alpha, bin_fill_holes,
                crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                aug_scale_non_uniform, aug_rot_mag,
                aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                mask_mode, mask_prop_range,
                cons_loss_fn, cons_weight, conf_thresh, conf_per_pixel, rampup, unsup_batch_ratio,
                num_epochs, iters_per_epoch, batch_size,
                n_sup, n_unsup, n_val, split_seed, split_path, val_seed, save_preds, save_model,
                num_workers,
                synthetic=False, synthetic_n_classes=21, synthetic_val_batches=2, compute_dtype='bf16',
                no_fuse_batches=False, synthetic_source_size='', deterministic=False,
                allreduce_dtype='fp32', step_options=None, **mask_options):
    """The body of the mask-driven mean-teacher commands: this one (box masks: CutMix / Cutout) and
    train_seg_semisup_cowmask_mt (CowMix / CowOut). `settings` is what the command prints; `make_mask_generator(prop_range)` -> the
    command's mask_gen.MaskGenerator. A generator with `generate_ranges` sends an int32 box table per batch (rasterised inside the
    kernels under `invert`); any other makes its masks on the device from host parameters (`torch_masks_from_params`) and the step
    takes the materialised mask. A generator that declares `needs_teacher` (mask_gen.ClassMixGenerator) makes its mask from the
    teacher's prediction on image 1, AFTER the unsupervised images are staged: one extra teacher pass under no_grad per
    unsupervised batch, outside the step (`mask_prop_range` is None for such a command: it has no share of ones to draw).
    `mask_options`: options of the command that only its generator reads. `step_options(n_classes, torch_device, world)`, when a
    command gives one, is called once the class count and the device are known -> (further StepConfig keywords, the command's
    `after_epoch(epoch_i)` hook or None) (train_seg_semisup_classthresh_mt)."""
    if mask_prop_range is None:
        pass
    elif ':' in mask_prop_range:
        lo, hi = mask_prop_range.split(':')
        mask_prop_range = (float(lo.strip()), float(hi.strip()))
    else:
        mask_prop_range = float(mask_prop_range)

    if mask_mode not in ('zero', 'mix'):
        raise ValueError('Unknown mask_mode {}'.format(mask_mode))

    import os
    import numpy as np
    import torch
    from . import lr_schedules, ops
    from .step import CutMixMeanTeacherStep, StepConfig, UnsupBatch

    crop = tc.parse_crop_size(crop_size)

    # Without --synthetic: the reference's data set path (:64-72), shared by the four trainers (trainer_common.py)
    ds_dict = tc.open_dataset(synthetic, crop, dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path)

    world, rank, torch_device = tc.setup_process(job_name, data_parallel=True)

    n_classes = int(synthetic_n_classes)
    run = None
    if ds_dict is not None:
        run = tc.DatasetRun(ds_dict, torch_device, batch_size)
        n_classes = run.n_classes
    nets = tc.build_networks(arch, n_classes, model, compute_dtype, torch_device, world, opt_type, learning_rate, sgd_momentum,
                             sgd_nesterov, sgd_weight_decay, teacher_alpha, freeze_bn, bin_fill_holes)
    if nets is None:
        return
    student_net, teacher_net, eval_net, student_optim, teacher_optim, dtype = nets

    mask_generator = make_mask_generator(mask_prop_range)
    box_tables = hasattr(mask_generator, 'generate_ranges')
    teacher_masks = bool(getattr(mask_generator, 'needs_teacher', False))
    if teacher_masks and mask_mode != 'mix':
        raise ValueError('a mask made from the teacher\'s prediction on image 1 needs --mask_mode mix')

    if iters_per_epoch == -1:
        iters_per_epoch = 1000 if run is None else run.iters_per_epoch(iters_per_epoch)
    schedulers = lr_schedules.make_lr_schedulers(
        optimizer=student_optim, total_iters=iters_per_epoch * num_epochs, schedule_type=lr_sched, step_epochs=lr_step_epochs,
        step_gamma=lr_step_gamma, poly_power=lr_poly_power)

    step_extra, after_epoch = step_options(n_classes, torch_device, world) if step_options is not None else ({}, None)
    step_cfg = StepConfig(mask_mode=mask_mode, cons_loss_fn=cons_loss_fn, cons_weight=cons_weight,
                          conf_thresh=conf_thresh, conf_per_pixel=conf_per_pixel, rampup=rampup,
                          unsup_batch_ratio=unsup_batch_ratio, invert=invert,
                          fuse_batches=not no_fuse_batches, compute_dtype=dtype,
                          deterministic=deterministic, allreduce_dtype=allreduce_dtype, **step_extra)
    step = CutMixMeanTeacherStep(student_net, teacher_net, student_optim, teacher_optim, step_cfg)

    # synthetic data: N(0,1) images, uniform labels with 5 % ignore, all-ones validity masks
    H, W = crop
    gen = torch.Generator(device=torch_device).manual_seed(12345 + rank)
    mask_rng = np.random.RandomState(12345 + rank)
    # masks made on the device draw their noise from a generator of their own (the data stream above stays what it is)
    noise_gen = None if (box_tables or teacher_masks) else torch.Generator(device=torch_device).manual_seed(12345 + rank)
    data = tc.SyntheticData(gen, batch_size, crop, n_classes, dtype)

    # `--synthetic_source_size h,w`: the synthetic samples are uint8 SOURCE images of that size resident in HBM and every
    # batch goes through the device-side input staging (device_pipeline.py: crop / Hung scale / flips / colour
    # augmentation / standardisation -- the reference's loader-worker transforms, :150-183, with the --aug_* options)
    augment = None
    if run is not None:
        # the data set path: the same staging, every sample gathered from its own (variable-sized) pool entry. The reference
        # seeds none of its numpy draws; neither does this path. The two unsupervised streams share one sampler (:203-212)
        mask_rng = np.random.RandomState()
        if noise_gen is not None:
            noise_gen.seed()
        augment = run.make_streams(student_net, (H, W), dtype, settings,
                                   0 if cons_weight <= 0.0 else (2 if step_cfg.mix else 1))
    elif synthetic_source_size:
        from .device_pipeline import DeviceAugmenter
        hs, ws = [int(v.strip()) for v in synthetic_source_size.split(',')]
        augment = DeviceAugmenter((H, W), student_net.MEAN, student_net.STD, out_dtype=dtype,
                                  rng=np.random.RandomState(54321 + rank), colour_rng=np.random.RandomState(99 + rank),
                                  **tc.augmenter_options(settings))
        src_pool = torch.randint(0, 256, (4 * batch_size, hs, ws, 3), generator=gen, device=torch_device, dtype=torch.uint8)
        lab_pool = torch.randint(0, n_classes, (4 * batch_size, hs, ws), generator=gen, device=torch_device).to(torch.uint8)
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

    def make_mask():
        """one batch of masks, outside any graph capture -> the `ranges=` or `mask=` argument of UnsupBatch"""
        if box_tables:
            return dict(ranges=ops.ranges_to_device(mask_generator.generate_ranges(batch_size, (H, W), rng=mask_rng), torch_device))
        params = mask_generator.generate_params(batch_size, (H, W), rng=mask_rng)
        return dict(mask=mask_generator.torch_masks_from_params(params, (H, W), torch_device, generator=noise_gen))

    def make_teacher_mask(x1_tea, um1):
        """the mask of a `needs_teacher` generator: the teacher's low-resolution logits of image 1 under no_grad -- the pass the step
        repeats --, then the generator's kernels at the step's own output size and corner convention. The pass must leave the
        teacher as it found it (teacher_prepass_moves)"""
        keys = mask_generator.generate_params(batch_size, n_classes, rng=mask_rng)
        with torch.no_grad():
            logits = teacher_net.forward_lowres(x1_tea)
        return dict(mask=mask_generator.torch_masks_from_logits(keys, logits, (H, W), step.align_corners, valid=um1))

    if teacher_masks:
        moved = teacher_prepass_moves(teacher_net, freeze_bn)
        if moved:
            raise ValueError(moved)

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
                mask_arg = None if teacher_masks else make_mask()
                if augment is not None:
                    if run is not None:
                        u0 = augment.stage(run.pool, next(unsup_iter_0), False)
                        u1 = augment.stage(run.pool, next(unsup_iter_1), False) if step_cfg.mix else None
                    else:
                        u0 = staged(False)
                        u1 = staged(False) if step_cfg.mix else None
                    if teacher_masks:
                        mask_arg = make_teacher_mask(u1['image'], u1['mask'])
                    unsup.append(UnsupBatch(u0['image'], um0=u0['mask'],
                                            x1_tea=None if u1 is None else u1['image'],
                                            um1=None if u1 is None else u1['mask'], x0_stu=u0.get('image_stu'),
                                            x1_stu=None if u1 is None else u1.get('image_stu'), **mask_arg))
                    continue
                x0 = data.images()
                x1 = data.images() if step_cfg.mix else None
                x0s = data.images() if aug_strong_colour else None
                x1s = data.images() if (aug_strong_colour and step_cfg.mix) else None
                if teacher_masks:
                    mask_arg = make_teacher_mask(x1, None)
                unsup.append(UnsupBatch(x0, x1_tea=x1, x0_stu=x0s, x1_stu=x1s, **mask_arg))
        return batch_x, batch_y, unsup

    evaluate = run.evaluate_with(eval_net, step) if run is not None else data.evaluate_with(eval_net, step, synthetic_val_batches)
    # inherited, not chosen: the confusion matrix is all_reduced and only rank 0 prints; these are the trainers with the img/s line
    if not tc.run_epochs(step, make_batch, evaluate, student_net, teacher_net, eval_net, schedulers, num_epochs,
                         iters_per_epoch, freeze_bn, rampup, conf_thresh, n_classes, bin_fill_holes, torch_device,
                         data_parallel=True, rank=rank, nan_checks_consistency=nan_checks_consistency, polls_step_nan=polls_step_nan,
                         img_per_s_of=(batch_size, world), after_epoch=after_epoch):
        return

    # inherited, not chosen: the whole module through checkpoint.save_model (the VAT trainer writes a state_dict)
    if save_model and rank == 0 and submit_config.run_dir is not None:
        # the reference pickles the whole module (:533-535): a clean replica without this build's runtime state, under
        # the reference's class paths (checkpoint.py)
        from . import checkpoint
        model_path = os.path.join(submit_config.run_dir, 'model.pth')
        checkpoint.save_model(eval_net, model_path)

    if run is not None:
        run.finish(eval_net, step, save_preds, submit_config, bin_fill_holes)       # :537-577


experiment = tc.make_command(train_seg_semisup_mask_mt, (
    tc.head_options(sgd_nesterov=False) + tc.geometry_options() + tc.colour_options() +
    [click.option('--mask_mode', type=click.Choice(['zero', 'mix']), default='mix'),
     click.option('--mask_prop_range', type=str, default='0.5'),
     click.option('--boxmask_n_boxes', type=int, default=1),
     click.option('--boxmask_fixed_aspect_ratio', is_flag=True, default=False),
     click.option('--boxmask_by_size', is_flag=True, default=False),
     click.option('--boxmask_outside_bounds', is_flag=True, default=False),
     click.option('--boxmask_no_invert', is_flag=True, default=False)] +
    tc.consistency_options() +
    tc.run_options(after_val_seed=[click.option('--synthetic_source_size', type=str, default='')]) +
    tc.build_options() +
    [click.option('--no_fuse_batches', is_flag=True, default=False),
     # run-to-run deterministic weight gradients (slab + ordered reduce instead of fp32 atomics; 1.5-2 % slower)
     click.option('--deterministic', is_flag=True, default=False),
     # data-parallel gradient exchange: the fp32 arena (default) or a bf16 staging copy (half the bytes on xGMI)
     click.option('--allreduce_dtype', type=click.Choice(['fp32', 'bf16']), default='fp32')]))


if __name__ == '__main__':
    experiment()
