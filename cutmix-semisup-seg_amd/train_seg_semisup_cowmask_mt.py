"""
CowMix / CowOut mean-teacher (or Pi-model) trainer: train_seg_semisup_mask_mt with CowMask in the place of the box mask. The
reference has no such program; its mask_gen.py carries the scaffolding (an abstract `torch_masks_from_params`, `gaussian_kernels`) of
the generator its authors published next (French, Oliver, Salimans, "Milking CowMask for semi-supervised image classification").

The option table is the CutMix trainer's with the five `--boxmask_*` options replaced, in place, by `--cow_sigma_range`; everything else
-- data sources, `--mask_mode mix` (CowMix) / `zero` (CowOut), data parallelism, `--deterministic`, `--save_model`, `--save_preds`, the
log -- is that trainer's, because the job body is that trainer's (train_seg_semisup_mask_mt.mask_mt_job). Per unsupervised batch the
host draws a share p of ones and a Gaussian sigma per sample (`--mask_prop_range`, `--cow_sigma_range`, log-uniform); the noise, its
fp64 blur, statistics and threshold run on the device (mask_gen.CowMaskGenerator, csrc/cowmask.hip), outside any graph capture, and
the step takes the materialised mask: 1 = "take image 1" (mix) / "keep" (zero). The defaults, `0.2:0.8` and `4:16`, are the paper's
small-image CowMix setting as far as we recall it; neither has been tuned on these data sets.
"""
import click

from . import job_helper, trainer_common as tc
from .train_seg_semisup_mask_mt import mask_mt_job


def parse_range(text, what):
    """'lo:hi' or one number -> (lo, hi)"""
    try:
        parts = [float(v.strip()) for v in str(text).split(':')]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2):
        raise ValueError('{} {!r}: expected lo:hi or one number'.format(what, text))
    return (parts[0], parts[-1])


@job_helper.job('train_seg_semisup_cowmask_mt', enumerate_job_names=False)
def train_seg_semisup_cowmask_mt(submit_config, dataset, model, arch, freeze_bn,
                                 opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                                 learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                                 teacher_alpha, bin_fill_holes,
                                 crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                                 aug_scale_non_uniform, aug_rot_mag,
                                 aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                                 aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                                 mask_mode, mask_prop_range,
                                 cow_sigma_range,
                                 cons_loss_fn, cons_weight, conf_thresh, conf_per_pixel, rampup, unsup_batch_ratio,
                                 num_epochs, iters_per_epoch, batch_size,
                                 n_sup, n_unsup, n_val, split_seed, split_path, val_seed, save_preds, save_model,
                                 num_workers,
                                 synthetic=False, synthetic_n_classes=21, synthetic_val_batches=2, compute_dtype='bf16',
                                 no_fuse_batches=False, synthetic_source_size='', deterministic=False,
                                 allreduce_dtype='fp32'):
    settings = locals().copy()
    del settings['submit_config']

    # refused here, before the data set is opened or the GPU is touched
    from . import mask_gen
    sigma_range = parse_range(cow_sigma_range, '--cow_sigma_range')
    mask_gen.CowMaskGenerator(parse_range(mask_prop_range, '--mask_prop_range'), sigma_range)

    def cow_masks(prop_range):
        return mask_gen.CowMaskGenerator(prop_range, sigma_range)

    # as the CutMix trainer, whose body this is: a NaN supervised loss ends the job, the step's NaN flag is polled every iteration
    return mask_mt_job('train_seg_semisup_cowmask_mt', submit_config, settings, cow_masks, invert=True,
                       nan_checks_consistency=False, polls_step_nan=True, **settings)


experiment = tc.make_command(train_seg_semisup_cowmask_mt, (
    tc.head_options(sgd_nesterov=False) + tc.geometry_options() + tc.colour_options() +
    [click.option('--mask_mode', type=click.Choice(['zero', 'mix']), default='mix'),
     click.option('--mask_prop_range', type=str, default='0.2:0.8'),
     click.option('--cow_sigma_range', type=str, default='4:16')] +
    tc.consistency_options() +
    tc.run_options(after_val_seed=[click.option('--synthetic_source_size', type=str, default='')]) +
    tc.build_options() +
    [click.option('--no_fuse_batches', is_flag=True, default=False),
     click.option('--deterministic', is_flag=True, default=False),
     click.option('--allreduce_dtype', type=click.Choice(['fp32', 'bf16']), default='fp32')]))


if __name__ == '__main__':
    experiment()
