"""
ClassMix mean-teacher (or Pi-model) trainer: train_seg_semisup_mask_mt with the mask cut along the teacher's own predicted class
regions of image 1 (Olsson, Tranheden, Pinto, Svensson, "ClassMix: Segmentation-Based Data Augmentation for Semi-Supervised
Learning", WACV 2021) in the place of the box mask. The reference has no such program.

The option table is the CutMix trainer's with the five `--boxmask_*` options and `--mask_prop_range` removed and nothing added: the
share of classes is fixed at ceil(m / 2) of the m classes the teacher predicts in the sample (the rule of the authors' published
code as far as we recall it; not tuned here). `--mask_mode` accepts only `mix`. Everything else -- data sources, data parallelism,
`--deterministic`, `--save_model`, `--save_preds`, the log -- is that trainer's, because the job body is that trainer's
(train_seg_semisup_mask_mt.mask_mt_job). Per unsupervised batch the host draws one key per sample and class
(mask_gen.ClassMixGenerator); after the unsupervised images are staged the teacher runs once over image 1 under no_grad, and the
full-resolution argmax of its logits, the classes present among the valid pixels, the half with the smallest keys and the membership
mask are made on the device (csrc/classmix.hip), outside any graph capture. The step takes the materialised mask: 1 = "take image 1".

That pre-pass repeats one of the teacher's two forward passes of the step, and it must leave the teacher exactly as it found it:
parameters, BatchNorm running statistics, dropout generator state. With `--freeze_bn` on the DeepLab v2 and U-Net families that holds
by itself; a configuration in which a training-mode pass would move running statistics or draw dropout noise (no `--freeze_bn`; the
DeepLab v3+ head, which stays on batch statistics) is refused before the GPU is touched.
"""
import click

from . import job_helper, trainer_common as tc
from .train_seg_semisup_mask_mt import mask_mt_job, teacher_prepass_moves


def refuse_a_moving_prepass(arch, freeze_bn):
    """ValueError when the teacher's pre-pass would change the teacher, decided on a replica that never leaves the host"""
    if not freeze_bn:
        raise ValueError('train_seg_semisup_classmix_mt makes its mask from a teacher pass before the step, which must not move the '
                         'teacher\'s BatchNorm running statistics: run with --freeze_bn')
    import torch
    from .architectures import network_architectures
    with torch.random.fork_rng(devices=[]):              # the replica's initialisation leaves the host's random stream alone
        probe = network_architectures.seg.get(arch)(2, pretrained=False)
    if not hasattr(probe, 'freeze_batchnorm'):
        raise ValueError('Network {} does not support batchnorm freezing'.format(arch))
    why = teacher_prepass_moves(probe, freeze_bn)
    if why:
        raise ValueError('train_seg_semisup_classmix_mt --arch {}: {}'.format(arch, why))


@job_helper.job('train_seg_semisup_classmix_mt', enumerate_job_names=False)
def train_seg_semisup_classmix_mt(submit_config, dataset, model, arch, freeze_bn,
                                  opt_type, sgd_momentum, sgd_nesterov, sgd_weight_decay,
                                  learning_rate, lr_sched, lr_step_epochs, lr_step_gamma, lr_poly_power,
                                  teacher_alpha, bin_fill_holes,
                                  crop_size, aug_hflip, aug_vflip, aug_hvflip, aug_scale_hung, aug_max_scale,
                                  aug_scale_non_uniform, aug_rot_mag,
                                  aug_strong_colour, aug_colour_brightness, aug_colour_contrast, aug_colour_saturation,
                                  aug_colour_hue, aug_colour_prob, aug_colour_greyscale_prob,
                                  mask_mode,
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
    if mask_mode != 'mix':
        raise ValueError('train_seg_semisup_classmix_mt: --mask_mode {} is not built (only mix)'.format(mask_mode))
    refuse_a_moving_prepass(arch, freeze_bn)

    def class_masks(prop_range):
        from . import mask_gen
        return mask_gen.ClassMixGenerator()

    # as the CutMix trainer, whose body this is: a NaN supervised loss ends the job, the step's NaN flag is polled every iteration
    return mask_mt_job('train_seg_semisup_classmix_mt', submit_config, settings, class_masks, invert=True,
                       nan_checks_consistency=False, polls_step_nan=True, mask_prop_range=None, **settings)


experiment = tc.make_command(train_seg_semisup_classmix_mt, (
    tc.head_options(sgd_nesterov=False) + tc.geometry_options() + tc.colour_options() +
    [click.option('--mask_mode', type=click.Choice(['mix']), default='mix')] +
    tc.consistency_options() +
    tc.run_options(after_val_seed=[click.option('--synthetic_source_size', type=str, default='')]) +
    tc.build_options() +
    [click.option('--no_fuse_batches', is_flag=True, default=False),
     click.option('--deterministic', is_flag=True, default=False),
     click.option('--allreduce_dtype', type=click.Choice(['fp32', 'bf16']), default='fp32')]))


if __name__ == '__main__':
    experiment()
