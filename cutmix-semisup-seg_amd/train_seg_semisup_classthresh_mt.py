"""
Class-threshold CutMix mean-teacher (or Pi-model) trainer: train_seg_semisup_mask_mt with the one confidence threshold of its
consistency loss replaced by one threshold per class -- typed as a list from eval_seg's per-threshold pseudo-label report, or
self-adaptive after FreeMatch (Wang, Chen, Heng, Hou, Fan, Wu, Wang, Savvides, Shinozaki, Raj, Schiele, Xie, "FreeMatch:
Self-adaptive Thresholding for Semi-supervised Learning", ICLR 2023) without its fairness loss. The reference has no such program.

The option table is the CutMix trainer's plus
    --class_thresh   `freematch` (default), or C comma-separated numbers in (0, 1]: static thresholds, one per class
    --thresh_ema     the EMA momentum of the self-adaptive thresholds (0.999; in [0, 1))
    --thresh_floor   their lower clamp (0.0)
and `--conf_thresh` (0.97; > 0) is their CEILING: 1 gives plain FreeMatch. A pixel passes when the teacher's confidence reaches the
threshold of the class it predicts; that bit stands wherever the CutMix trainer compares with `--conf_thresh` (the rate of the default
mode, the factor of `--conf_per_pixel`). The self-adaptive thresholds start at 1 / C (everything passes) and are re-made once per
iteration, on the device and without a host synchronisation, from sums that ride in the loss launch (csrc/cthresh.hip);
the thresholds an iteration applies are made from the iterations before it. One process only: the statistics are not exchanged.

Everything else -- masks, data sources, `--deterministic`, `--save_model` (model.pth is the CutMix trainer's: eval_seg scores it as it
is), the log -- is that trainer's, because the job body is (train_seg_semisup_mask_mt.mask_mt_job). After each epoch's lines come
    -- class thresholds tau=0.812: 0.812, 0.455, ...
    -- class pass rate 71.2%, 12.5%, -, ...         (`-`: the teacher never predicted the class on a valid pixel)
"""
import os

import click

from . import job_helper, trainer_common as tc
from .train_seg_semisup_mask_mt import mask_mt_job


def checked_options(class_thresh, thresh_ema, thresh_floor, conf_thresh, n_classes=None):
    """The command's own options, checked on the host -> (mode, ema, floor); ValueError names the option."""
    from .ops import parse_class_thresh
    try:
        mode = parse_class_thresh(class_thresh, n_classes)
    except ValueError as e:
        raise ValueError('--class_thresh: {}'.format(e))
    if not (0.0 < float(conf_thresh) <= 1.0):
        raise ValueError('--conf_thresh is the ceiling of the class thresholds: it must be in (0, 1], got {}'.format(conf_thresh))
    if mode != 'freematch':
        for name, v in (('--thresh_ema', thresh_ema), ('--thresh_floor', thresh_floor)):
            if v is not None:
                raise ValueError('{} belongs to --class_thresh freematch; a static list has nothing to adapt'.format(name))
        return mode, 0.0, 0.0
    ema = 0.999 if thresh_ema is None else float(thresh_ema)
    floor = 0.0 if thresh_floor is None else float(thresh_floor)
    if not (0.0 <= ema < 1.0):
        raise ValueError('--thresh_ema must be in [0, 1), got {}'.format(thresh_ema))
    if not (0.0 <= floor <= 1.0):
        raise ValueError('--thresh_floor must be in [0, 1], got {}'.format(thresh_floor))
    if floor > float(conf_thresh):
        raise ValueError('--thresh_floor {} lies above the ceiling --conf_thresh {}'.format(floor, conf_thresh))
    return mode, ema, floor


def format_report(rep):
    """the two lines behind an epoch's log lines"""
    thr = ', '.join('{:.3f}'.format(float(v)) for v in rep['thr'])
    rate = ', '.join('-' if r is None else '{:.1f}%'.format(100.0 * r) for r in rep['pass_rate'])
    return ['-- class thresholds tau={:.3f}: {}'.format(rep['tau'], thr), '-- class pass rate {}'.format(rate)]


@job_helper.job('train_seg_semisup_classthresh_mt', enumerate_job_names=False)
def train_seg_semisup_classthresh_mt(submit_config, dataset, model, arch, freeze_bn,
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
                                     allreduce_dtype='fp32', class_thresh='freematch', thresh_ema=None, thresh_floor=None):
    settings = locals().copy()
    del settings['submit_config']

    # refused here, before the data set is opened or the GPU is touched
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise ValueError('train_seg_semisup_classthresh_mt runs as one process: the data-parallel exchange of the threshold '
                         'statistics is not implemented (WORLD_SIZE={})'.format(os.environ.get('WORLD_SIZE')))
    mode, ema, floor = checked_options(class_thresh, thresh_ema, thresh_floor, conf_thresh,
                                       int(synthetic_n_classes) if synthetic else None)

    own = ('class_thresh', 'thresh_ema', 'thresh_floor')
    common = {k: v for k, v in settings.items() if not k.startswith('boxmask_') and k not in own}

    def box_masks(prop_range):
        from . import mask_gen
        return mask_gen.BoxMaskGenerator(prop_range=prop_range, n_boxes=boxmask_n_boxes,
                                         random_aspect_ratio=not boxmask_fixed_aspect_ratio, prop_by_area=not boxmask_by_size,
                                         within_bounds=not boxmask_outside_bounds, invert=not boxmask_no_invert)

    def step_options(n_classes, torch_device, world):
        from . import ops
        if world > 1:
            raise ValueError('train_seg_semisup_classthresh_mt runs as one process')
        try:
            # (a static list against the class count of a data set, known only now)
            ct = ops.ClassThresholds(n_classes, torch_device, mode=mode, ema=ema, floor=floor, ceil=float(conf_thresh))
        except ValueError as e:
            raise ValueError('--class_thresh: {}'.format(e))

        def after_epoch(epoch_i):
            ct.update()                     # the epoch's last iteration into the counters (and the thresholds) before they are read
            for line in format_report(ct.pop_epoch_report()):
                print(line)
        return dict(class_thresh=ct), after_epoch

    # as the CutMix trainer, whose body this is: a NaN supervised loss ends the job, the step's NaN flag is polled every iteration
    return mask_mt_job('train_seg_semisup_classthresh_mt', submit_config, settings, box_masks, invert=not boxmask_no_invert,
                       nan_checks_consistency=False, polls_step_nan=True, step_options=step_options, **common)


experiment = tc.make_command(train_seg_semisup_classthresh_mt, (
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
     click.option('--deterministic', is_flag=True, default=False),
     click.option('--allreduce_dtype', type=click.Choice(['fp32', 'bf16']), default='fp32'),
     click.option('--class_thresh', type=str, default='freematch'),
     # (no default here: given beside a static list they are refused)
     click.option('--thresh_ema', type=float, default=None),
     click.option('--thresh_floor', type=float, default=None)]))


if __name__ == '__main__':
    experiment()
