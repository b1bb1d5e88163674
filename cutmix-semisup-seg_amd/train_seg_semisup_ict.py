"""
Mirror of the reference's train_seg_semisup_ict.py: the ICT (interpolation consistency training) mean-teacher (or
Pi-model) trainer with the same 50 command-line options (names and defaults, train_seg_semisup_ict.py:508-559), job/log
layout and per-epoch log lines, driving the MI355X ICT iteration (ict.py).

`--synthetic` (plus `--synthetic_n_classes`, `--synthetic_val_batches`) trains on synthetic tensors of the crop shape;
`--compute_dtype` as in the other trainers. Without `--synthetic`, `--dataset` (Pascal VOC, CamVid, Cityscapes, ISIC 2017) trains on what `./semantic_segmentation.cfg` locates, through the
data set path the four trainers share (trainer_common.open_dataset / DatasetRun, as in train_seg_semisup_mask_mt.py): the
reference's splits and index streams on the host, every image decoded once into an HBM-resident pool, training crops and padded
evaluation batches gathered on the device; VAL mIoU every epoch, `--save_preds`, FINAL TEST with `--n_val`. One GPU, a
`--crop_size` is required; the other data sets, `--crop_size ''` and WORLD_SIZE > 1 stop with a message before the GPU is touched.
An unsupervised step takes two consecutive batches of the one unsupervised iterator (:272-273), each with its validity mask and,
under `--aug_strong_colour`, its student view. The option blocks, set-up, networks, data set path and epoch loop it shares with the
other three trainers are in trainer_common.py; losses are accumulated on the device. One GPU: the ICT step has no data-parallel
form yet and refuses WORLD_SIZE > 1.
"""
import click

from . import job_helper, trainer_common as tc


@job_helper.job('train_seg_semisup_ict', enumerate_job_names=False)
def train_seg_semisup_ict(submit_config, dataset, model, arch, freeze_bn,
                          opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                          learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                          teacher_alpha, bin_fill_holes,
                          crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                          aug_scale_non_uniform, aug_rot_mag,
                          aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                          aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                          ict_alpha, cons_loss_fn, cons_weight, conf_thresh, conf_per_pixel, rampup, unsup_batch_ratio,
                          num_epochs, iters_per_epoch, batch_size,
                          n_sup, n_unsup, n_val, split_seed, split_path, val_seed, save_preds, save_model,
                          num_workers,
                          synthetic=False, synthetic_n_classes=21, synthetic_val_batches=2, compute_dtype='bf16'):
    settings = locals().copy()
    del settings['submit_config']

    import os
    import numpy as np
    import torch
    from . import lr_schedules
    from .ict import ICTMeanTeacherStep, ICTConfig, ICTUnsupBatch

    crop = tc.parse_crop_size(crop_size)
    # Without --synthetic: the data set path the four trainers share (trainer_common.py); refusals come first
    ds_dict = tc.open_dataset(synthetic, crop, dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path)
    # inherited, not chosen: the ICT step has no data-parallel form, so more than one process is refused
    world, _, torch_device = tc.setup_process('train_seg_semisup_ict', data_parallel=False, one_gpu_what='ICT')

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

    if iters_per_epoch == -1:
        iters_per_epoch = 1000 if run is None else run.iters_per_epoch(iters_per_epoch)
    schedulers = lr_schedules.make_lr_schedulers(
        optimizer=student_optim, total_iters=iters_per_epoch * num_epochs, schedule_type=lr_sched, step_epochs=lr_step_epochs,
        step_gamma=lr_step_gamma, poly_power=lr_poly_power)

    cfg = ICTConfig(ict_alpha=ict_alpha, cons_loss_fn=cons_loss_fn, cons_weight=cons_weight, conf_thresh=conf_thresh,
                    conf_per_pixel=conf_per_pixel, rampup=rampup, unsup_batch_ratio=unsup_batch_ratio)
    # inherited, not chosen: every process seeds 12345 (the VAT and CutMix trainers add their rank)
    data = tc.SyntheticData(torch.Generator(device=torch_device).manual_seed(12345), batch_size, crop, n_classes, dtype)
    step = ICTMeanTeacherStep(student_net, teacher_net, student_optim, teacher_optim, cfg, rng=np.random.RandomState(12345))

    augment = None
    if run is not None:
        augment = run.make_streams(student_net, crop, dtype, settings, 1 if cons_weight > 0.0 else 0)

    def make_batch():
        if run is not None:
            sb = augment.stage(run.pool, next(sup_iter), True)
            unsup = []
            if cons_weight > 0.0:
                for _r in range(unsup_batch_ratio):
                    # two consecutive batches of the one unsupervised iterator per blend (:272-273)
                    u0 = augment.stage(run.pool, next(unsup_iter), False)
                    u1 = augment.stage(run.pool, next(unsup_iter), False)
                    unsup.append(ICTUnsupBatch(u0['image'], u1['image'], um0=u0['mask'], um1=u1['mask'],
                                               x0_stu=u0.get('image_stu'), x1_stu=u1.get('image_stu')))
            return sb['image'], sb['labels'], unsup
        batch_x, batch_y = data.images(), data.labels()
        unsup = []
        if cons_weight > 0.0:
            for _r in range(unsup_batch_ratio):
                # two unsupervised batches per blend (:272-273); paired (weak / strong) samples under --aug_strong_colour
                x0, x1 = data.images(), data.images()
                unsup.append(ICTUnsupBatch(x0, x1, x0_stu=data.images() if aug_strong_colour else None,
                                           x1_stu=data.images() if aug_strong_colour else None))
        return batch_x, batch_y, unsup

    tc.print_settings(settings)
    if run is None:
        tc.print_synthetic_dataset(crop, n_classes, world)
    else:
        sup_iter, unsup_iter = (run.print_sizes_and_start(n_sup) + [None])[:2]

    # inherited, not chosen: a NaN supervised OR consistency loss ends the job, the step's NaN flag is not polled; no all_reduce
    # of the confusion matrix and no rank gate on the prints (one process); no img/s line
    evaluate = run.evaluate_with(eval_net, step) if run is not None else data.evaluate_with(eval_net, step, synthetic_val_batches)
    if not tc.run_epochs(step, make_batch, evaluate, student_net, teacher_net, eval_net, schedulers, num_epochs,
                         iters_per_epoch, freeze_bn, rampup, conf_thresh, n_classes, bin_fill_holes, torch_device,
                         data_parallel=False, nan_checks_consistency=True, polls_step_nan=False):
        return

    # inherited, not chosen: the whole module through checkpoint.save_model (the VAT trainer writes a state_dict)
    if save_model and submit_config.run_dir is not None:
        # the reference pickles the whole module (:460-462): a clean replica under the reference's class paths (checkpoint.py)
        from . import checkpoint
        checkpoint.save_model(eval_net, os.path.join(submit_config.run_dir, 'model.pth'))

    if run is not None:
        run.finish(eval_net, step, save_preds, submit_config, bin_fill_holes)       # :464-504


experiment = tc.make_command(train_seg_semisup_ict, (
    tc.head_options(sgd_nesterov=True) + tc.geometry_options() + tc.colour_options() +
    [click.option('--ict_alpha', type=float, default=0.1)] +
    tc.consistency_options(cons_weight=0.3) + tc.run_options() + tc.build_options()))


if __name__ == '__main__':
    experiment()
