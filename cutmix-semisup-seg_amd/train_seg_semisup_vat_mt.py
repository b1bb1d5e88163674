"""
Mirror of the reference's train_seg_semisup_vat_mt.py: the VAT mean-teacher (or Pi-model) trainer with the same 52
command-line options (names and defaults, train_seg_semisup_vat_mt.py:592-644), job/log layout and per-epoch log
lines, driving the MI355X VAT iteration (vat.py). SURVEY.md 8(f) rank 2.

`--synthetic` (plus `--synthetic_n_classes`, `--synthetic_val_batches`) trains on synthetic tensors of the crop shape, one
process per GPU under torchrun; `--compute_dtype` as in the other trainers. Without `--synthetic`, `--dataset` (Pascal VOC, CamVid, Cityscapes, ISIC 2017) trains on what `./semantic_segmentation.cfg` locates, through the
data set path the four trainers share (trainer_common.open_dataset / DatasetRun, as in train_seg_semisup_mask_mt.py): the
reference's splits and index streams on the host, every image decoded once into an HBM-resident pool, training crops and padded
evaluation batches gathered on the device; VAL mIoU every epoch, `--save_preds`, FINAL TEST with `--n_val`. One GPU, a
`--crop_size` is required; the other data sets, `--crop_size ''` and WORLD_SIZE > 1 stop with a message before the GPU is touched.
The option blocks, set-up, networks, data set path and epoch loop it shares with the other three trainers are in trainer_common.py,
losses are accumulated on the device.
The reference runs this trainer with its DenseNet-161 U-Net (BASELINE configs[4]); that backbone's arithmetic lives in
torchvision and is not part of this build -- the trainer takes any registered architecture, as the reference's does.
"""
import click

from . import job_helper, trainer_common as tc


@job_helper.job('train_seg_semisup_vat_mt', enumerate_job_names=False)
def train_seg_semisup_vat_mt(submit_config, dataset, model, arch, freeze_bn,
                             opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                             learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                             teacher_alpha, bin_fill_holes,
                             crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                             aug_scale_non_uniform, aug_rot_mag,
                             aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                             aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                             vat_radius, adaptive_vat_radius, vat_dir_from_student,
                             cons_loss_fn, cons_weight, conf_thresh, conf_per_pixel, rampup, unsup_batch_ratio,
                             num_epochs, iters_per_epoch, batch_size,
                             n_sup, n_unsup, n_val, split_seed, split_path, val_seed, save_preds, save_model,
                             num_workers,
                             synthetic=False, synthetic_n_classes=21, synthetic_val_batches=2, compute_dtype='bf16'):
    settings = locals().copy()
    del settings['submit_config']

    import os
    import torch
    from . import lr_schedules
    from .vat import VATMeanTeacherStep, VATConfig, VATUnsupBatch

    crop = tc.parse_crop_size(crop_size)
    # Without --synthetic: the data set path the four trainers share (trainer_common.py); refusals come first
    ds_dict = tc.open_dataset(synthetic, crop, dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path)
    world, rank, torch_device = tc.setup_process('train_seg_semisup_vat_mt', data_parallel=True)

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

    cfg = VATConfig(vat_radius=vat_radius, adaptive_vat_radius=adaptive_vat_radius, cons_loss_fn=cons_loss_fn,
                    cons_weight=cons_weight, conf_thresh=conf_thresh, conf_per_pixel=conf_per_pixel, rampup=rampup,
                    unsup_batch_ratio=unsup_batch_ratio)
    gen = torch.Generator(device=torch_device).manual_seed(12345 + rank)
    data = tc.SyntheticData(gen, batch_size, crop, n_classes, dtype)
    step = VATMeanTeacherStep(student_net, teacher_net, student_optim, teacher_optim, cfg,
                              vat_dir_from_student=vat_dir_from_student, generator=gen)

    augment = None
    if run is not None:
        augment = run.make_streams(student_net, crop, dtype, settings, 1 if cons_weight > 0.0 else 0)

    def make_batch():
        if run is not None:
            sb = augment.stage(run.pool, next(sup_iter), True)
            unsup = []
            if cons_weight > 0.0:
                for _r in range(unsup_batch_ratio):
                    u = augment.stage(run.pool, next(unsup_iter), False)                  # :369
                    unsup.append(VATUnsupBatch(u['image'], u.get('image_stu'), um=u['mask']))
            return sb['image'], sb['labels'], unsup
        batch_x, batch_y = data.images(), data.labels()
        unsup = []
        if cons_weight > 0.0:
            for _r in range(unsup_batch_ratio):
                x_tea = data.images()
                unsup.append(VATUnsupBatch(x_tea, data.images() if aug_strong_colour else None))
        return batch_x, batch_y, unsup

    tc.print_settings(settings)
    if run is None:
        tc.print_synthetic_dataset(crop, n_classes, world)
    else:
        sup_iter, unsup_iter = (run.print_sizes_and_start(n_sup) + [None])[:2]

    # inherited, not chosen: a NaN supervised OR consistency loss ends the job, the step's NaN flag is not polled; the confusion
    # matrix is all_reduced and only rank 0 prints (the ICT and augmentation trainers do neither); no img/s line
    evaluate = run.evaluate_with(eval_net, step) if run is not None else data.evaluate_with(eval_net, step, synthetic_val_batches)
    if not tc.run_epochs(step, make_batch, evaluate, student_net, teacher_net, eval_net, schedulers, num_epochs,
                         iters_per_epoch, freeze_bn, rampup, conf_thresh, n_classes, bin_fill_holes, torch_device,
                         data_parallel=True, rank=rank, nan_checks_consistency=True, polls_step_nan=False):
        return

    # inherited, not chosen: this trainer writes a state_dict, the other three go through checkpoint.save_model
    if save_model and rank == 0 and submit_config.run_dir is not None:
        torch.save(eval_net.state_dict(), os.path.join(submit_config.run_dir, 'model.pth'))

    if run is not None:
        run.finish(eval_net, step, save_preds, submit_config, bin_fill_holes)       # :547-587


experiment = tc.make_command(train_seg_semisup_vat_mt, (
    tc.head_options(sgd_nesterov=True) + tc.geometry_options() + tc.colour_options() +
    [click.option('--vat_radius', type=float, default=0.5),
     click.option('--adaptive_vat_radius', is_flag=True, default=False),
     click.option('--vat_dir_from_student', is_flag=True, default=False)] +
    tc.consistency_options(cons_loss_fns=('var', 'bce', 'kld', 'logits_var'), cons_loss_fn='kld') +
    tc.run_options() + tc.build_options()))


if __name__ == '__main__':
    experiment()
