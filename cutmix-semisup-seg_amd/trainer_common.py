"""
What the four semi-supervised trainers (train_seg_semisup_mask_mt / _vat_mt / _ict / _aug_mt) have in common: the shared blocks
of the reference's option tables, process and device set-up, networks and optimisers, synthetic data, and the epoch loop with
its bookkeeping and log lines. A trainer file keeps what is its own: its options, its config / step / batch construction and how
it saves.

Plain functions and one small class; what differs between trainers is a keyword argument or a callable passed in. torch is
imported inside the functions, as in the trainers: importing a trainer (its command line, its configuration errors) loads no
torch.
"""
import click

from . import job_helper


# ------------------------------------------------------------------------------------------------------------------
# the option table: the blocks of the reference's tables that the trainers share, in the reference's order
def head_options(sgd_nesterov):
    """`--job_desc` ... `--bin_fill_holes`."""
    return [
        click.option('--job_desc', type=str, default=''),
        click.option('--dataset', type=click.Choice(['camvid', 'cityscapes', 'pascal', 'pascal_aug', 'isic2017']),
                     default='pascal_aug'),
        click.option('--model', type=click.Choice(['mean_teacher', 'pi']), default='mean_teacher'),
        click.option('--arch', type=str, default='resnet101_deeplab_imagenet'),
        click.option('--freeze_bn', is_flag=True, default=False),
        click.option('--opt_type', type=click.Choice(['adam', 'sgd']), default='adam'),
        click.option('--sgd_momentum', type=float, default=0.9),
        click.option('--sgd_nesterov', is_flag=True, default=sgd_nesterov),
        click.option('--sgd_weight_decay', type=float, default=5e-4),
        click.option('--learning_rate', type=float, default=1e-4),
        click.option('--lr_sched', type=click.Choice(['none', 'stepped', 'cosine', 'poly']), default='none'),
        click.option('--lr_step_epochs', type=str, default=''),
        click.option('--lr_step_gamma', type=float, default=0.1),
        click.option('--lr_poly_power', type=float, default=0.9),
        click.option('--teacher_alpha', type=float, default=0.99),
        click.option('--bin_fill_holes', is_flag=True, default=False),
    ]


def geometry_options(after_crop_size=(), after_rot_mag=()):
    """`--crop_size` ... `--aug_rot_mag`; the augmentation trainer has an option of its own in each of the two places."""
    return [
        click.option('--crop_size', type=str, default='321,321'),
        *after_crop_size,
        click.option('--aug_hflip', is_flag=True, default=False),
        click.option('--aug_vflip', is_flag=True, default=False),
        click.option('--aug_hvflip', is_flag=True, default=False),
        click.option('--aug_scale_hung', is_flag=True, default=False),
        click.option('--aug_max_scale', type=float, default=1.0),
        click.option('--aug_scale_non_uniform', is_flag=True, default=False),
        click.option('--aug_rot_mag', type=float, default=0.0),
        *after_rot_mag,
    ]


def colour_options():
    """`--aug_strong_colour` ... `--aug_colour_greyscale_prob`."""
    return [
        click.option('--aug_strong_colour', is_flag=True, default=False),
        click.option('--aug_colour_brightness', type=float, default=0.4),
        click.option('--aug_colour_contrast', type=float, default=0.4),
        click.option('--aug_colour_saturation', type=float, default=0.4),
        click.option('--aug_colour_hue', type=float, default=0.1),
        click.option('--aug_colour_prob', type=float, default=0.8),
        click.option('--aug_colour_greyscale_prob', type=float, default=0.2),
    ]


def consistency_options(cons_loss_fns=('var', 'bce', 'kld', 'logits_var', 'logits_smoothl1'), cons_loss_fn='var',
                        cons_weight=1.0):
    """`--cons_loss_fn` ... `--unsup_batch_ratio`."""
    return [
        click.option('--cons_loss_fn', type=click.Choice(list(cons_loss_fns)), default=cons_loss_fn),
        click.option('--cons_weight', type=float, default=cons_weight),
        click.option('--conf_thresh', type=float, default=0.97),
        click.option('--conf_per_pixel', is_flag=True, default=False),
        click.option('--rampup', type=int, default=-1),
        click.option('--unsup_batch_ratio', type=int, default=1),
    ]


def run_options(after_val_seed=()):
    """`--num_epochs` ... `--num_workers`; the CutMix trainer has an option of its own after `--val_seed`."""
    return [
        click.option('--num_epochs', type=int, default=300),
        click.option('--iters_per_epoch', type=int, default=-1),
        click.option('--batch_size', type=int, default=10),
        click.option('--n_sup', type=int, default=100),
        click.option('--n_unsup', type=int, default=-1),
        click.option('--n_val', type=int, default=-1),
        click.option('--split_seed', type=int, default=12345),
        click.option('--split_path', type=click.Path(readable=True, exists=True)),
        click.option('--val_seed', type=int, default=131),
        *after_val_seed,
        click.option('--save_preds', is_flag=True, default=False),
        click.option('--save_model', is_flag=True, default=False),
        click.option('--num_workers', type=int, default=4),
    ]


def build_options():
    """The additions of this build that every trainer has."""
    return [
        click.option('--synthetic', is_flag=True, default=False),
        click.option('--synthetic_n_classes', type=int, default=21),
        click.option('--synthetic_val_batches', type=int, default=2),
        click.option('--compute_dtype', type=click.Choice(['bf16', 'fp32']), default='bf16'),
    ]


def make_command(job_fn, options):
    """The click command `experiment` of a trainer: `options` in order, every parameter handed to `job_fn.submit`."""
    def experiment(**params):
        job_fn.submit(**params)

    for opt in reversed(options):
        experiment = opt(experiment)
    return click.command()(experiment)


# ------------------------------------------------------------------------------------------------------------------
# checks that come before anything touches the GPU
def parse_crop_size(crop_size):
    return None if crop_size == '' else [int(x.strip()) for x in crop_size.split(',')]


def synthetic_crop(crop_size, synthetic):
    """`--crop_size` of a trainer that has no data set path: refuses to start without `--synthetic`."""
    crop = parse_crop_size(crop_size)
    if not synthetic:
        raise job_helper.JobNotRun('This build covers the training step, not the dataset pipeline (datapipe/, cv2, dataset ZIPs are out of '
              'scope and absent); run with --synthetic.')
    if crop is None:
        raise ValueError('--synthetic needs a --crop_size')
    return crop


# ------------------------------------------------------------------------------------------------------------------
# process and device set-up
def setup_process(job_name, data_parallel, one_gpu_what=None):
    """One process per GPU (WORLD_SIZE / RANK / LOCAL_RANK, as torchrun sets them): select the device -> (world, rank, device).
    With `data_parallel` more than one process brings up the process group; without it the trainer refuses them, naming
    `one_gpu_what` as what has no data-parallel form."""
    import os
    import torch
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1 and not data_parallel:
        raise RuntimeError('{} runs on one GPU: data-parallel {} is not implemented (WORLD_SIZE={})'.format(
            job_name, one_gpu_what, world))
    if not torch.cuda.is_available():
        raise RuntimeError('{} needs a GPU; there is no CPU fallback'.format(job_name))
    torch.cuda.set_device(local_rank)
    torch_device = torch.device('cuda', local_rank)
    if world > 1:
        import torch.distributed as dist
        from . import ops
        if not dist.is_initialized():
            dist.init_process_group('nccl')
        # RCCL creates its internal stream with the first collective; it occupies one of the four hardware queues. Probe the side
        # streams AFTER that, so the step's roles avoid the queue RCCL sits on (ops.probe_streams)
        _t = torch.ones(1, device=torch_device)
        dist.all_reduce(_t)
        torch.cuda.synchronize(torch_device)
        ops.probe_streams(torch_device, again=True)
    return world, rank, torch_device


# ------------------------------------------------------------------------------------------------------------------
# networks and optimisers
def build_networks(arch, n_classes, model, compute_dtype, torch_device, world, opt_type, learning_rate, sgd_momentum,
                   sgd_nesterov, sgd_weight_decay, teacher_alpha, freeze_bn, bin_fill_holes):
    """The student, the teacher (the student itself for the Pi model), their optimisers (the EMA update fused into the
    student's) -> (student_net, teacher_net, eval_net, student_optim, teacher_optim, dtype), or None after printing why the
    job ends here. Prints 'Loaded data' and 'Built network' where the trainers print them."""
    import torch
    from .architectures import network_architectures
    from . import optim_weight_ema, optim as fused_optim

    if bin_fill_holes and n_classes != 2:
        print('Binary hole filling can only be used with binary (2-class) segmentation datasets')
        return None
    print('Loaded data')

    NetClass = network_architectures.seg.get(arch)
    student_net = NetClass(n_classes, pretrained=False).to(torch_device)
    dtype = torch.bfloat16 if compute_dtype == 'bf16' else torch.float32
    student_net.compute_dtype = dtype
    if world > 1:
        import torch.distributed as dist
        for t in student_net.state_dict().values():       # identical replicas
            dist.broadcast(t, src=0)

    groups = [dict(params=list(student_net.pretrained_parameters()), lr=learning_rate * 0.1),
              dict(params=list(student_net.new_parameters()), lr=learning_rate)]
    if opt_type == 'adam':
        student_optim = fused_optim.FusedAdam(student_net, groups)
    elif opt_type == 'sgd':
        student_optim = fused_optim.FusedSGD(student_net, groups, momentum=sgd_momentum, nesterov=sgd_nesterov,
                                             weight_decay=sgd_weight_decay)
    else:
        raise ValueError('Unknown opt_type {}'.format(opt_type))

    if model == 'mean_teacher':
        teacher_net = NetClass(n_classes, pretrained=False).to(torch_device)
        teacher_net.compute_dtype = dtype
        for p in teacher_net.parameters():
            p.requires_grad = False
        teacher_optim = optim_weight_ema.EMAWeightOptimizer(teacher_net, student_net, teacher_alpha)
        teacher_optim.fuse_into(student_optim)
        eval_net = teacher_net
    elif model == 'pi':
        teacher_net = student_net
        teacher_optim = None
        eval_net = student_net
    else:
        print('Unknown model type {}'.format(model))
        return None

    if freeze_bn and not hasattr(student_net, 'freeze_batchnorm'):
        raise ValueError('Network {} does not support batchnorm freezing'.format(arch))
    print('Built network')
    return student_net, teacher_net, eval_net, student_optim, teacher_optim, dtype


# ------------------------------------------------------------------------------------------------------------------
# synthetic data
class SyntheticData(object):
    """N(0,1) images and uniform labels with 5 % ignore, of the crop's shape, drawn from `gen` on its device. Every call
    draws afresh: the number and order of the calls is what a seeded run reproduces."""

    def __init__(self, gen, batch_size, crop, n_classes, dtype):
        self.gen, self.batch_size, self.n_classes, self.dtype = gen, batch_size, n_classes, dtype
        self.H, self.W = crop

    def images(self):
        import torch
        return torch.randn(self.batch_size, 3, self.H, self.W, generator=self.gen, device=self.gen.device).to(self.dtype)

    def labels(self):
        import torch
        shape = (self.batch_size, 1, self.H, self.W)
        y = torch.randint(0, self.n_classes, shape, generator=self.gen, device=self.gen.device)
        y[torch.rand(shape, generator=self.gen, device=self.gen.device) < 0.05] = 255
        return y.to(torch.uint8)

    def evaluate_with(self, eval_net, step, n_batches):
        """-> the `evaluate(evaluator)` of run_epochs over `n_batches` fresh validation batches."""
        import torch

        def evaluate(evaluator):
            with torch.no_grad():
                for _b in range(n_batches):
                    vx, vy = self.images(), self.labels()
                    evaluator.sample_logits(eval_net.forward_lowres(vx), vy, (self.H, self.W), ignore_value=255,
                                            align_corners=step.align_corners)
        return evaluate


def print_settings(settings):
    """The 'Settings:' block and the 'Dataset:' heading after it."""
    print('Settings:')
    print(', '.join(['{}={}'.format(key, settings[key]) for key in sorted(list(settings.keys()))]))
    print('Dataset:')


def print_synthetic_dataset(crop, n_classes, world):
    print('synthetic: crop={}x{}, classes={}, world_size={}'.format(crop[0], crop[1], n_classes, world))


# ------------------------------------------------------------------------------------------------------------------
# the epoch loop
def accumulate(acc, res, n_unsup, ramp_val, conf_thresh, rampup):
    """Add one iteration's step results to the device-side sums `acc` (supervised loss, consistency loss, confidence rate; no
    host sync) -> the unsupervised batches this iteration counts for: `n_unsup`, or 0 when the step had no consistency loss."""
    acc[0] += res['sup_loss']
    if res['consistency_loss'] is None:
        return 0
    acc[1] += res['consistency_loss']
    if conf_thresh > 0.0:
        acc[2] += res['conf_rate']
    elif rampup > 0:
        acc[2] += ramp_val          # reference quirk (mask_mt:419-420): the rate column shows the ramp
    return n_unsup


def epoch_means(acc, n_sup_batches, n_unsup_batches):
    """The epoch's (supervised loss, consistency loss, confidence rate) from the sums: the one host sync of the epoch. All
    three are divided by the SUPERVISED batch count, as in the reference."""
    sums = acc.cpu().numpy()
    sup_loss = sums[0] / max(n_sup_batches, 1)
    consistency_loss = sums[1] / max(n_sup_batches, 1) if n_unsup_batches > 0 else 0.0
    conf_rate = sums[2] / max(n_sup_batches, 1) if n_unsup_batches > 0 else 0.0
    return sup_loss, consistency_loss, conf_rate


def network_dead(sup_loss, consistency_loss, nan_checks_consistency):
    import numpy as np
    return bool(np.isnan(sup_loss) or (nan_checks_consistency and np.isnan(consistency_loss)))


def epoch_line(epoch_i, seconds, sup_loss, consistency_loss, conf_rate, miou):
    return ('Epoch {}: took {:.3f}s, TRAIN clf loss={:.6f}, consistency loss={:.6f}, conf rate={:.3%}, '
            'VAL mIoU={:.3%}'.format(epoch_i + 1, seconds, sup_loss, consistency_loss, conf_rate, miou))


def run_epochs(step, make_batch, evaluate, student_net, teacher_net, eval_net, schedulers, num_epochs, iters_per_epoch,
               freeze_bn, rampup, conf_thresh, n_classes, bin_fill_holes, torch_device, data_parallel,
               nan_checks_consistency, polls_step_nan, rank=0, img_per_s_of=None):
    """'Training...' and the epochs: `step(*make_batch(), ramp_val=...)` per iteration with the losses summed on the device,
    then `evaluate(evaluator)` and the epoch's log lines -> False when the network died (said so; the job ends), else True.

      schedulers              (per-epoch, per-iteration) of lr_schedules.make_lr_schedulers
      data_parallel           sum the confusion matrix over the ranks and print on `rank` 0 only; without it every process prints
      nan_checks_consistency  a NaN consistency loss ends the job as a NaN supervised loss does
      polls_step_nan          ask `step.nan_detected()` before every iteration as well
      img_per_s_of            (batch_size, world) to print the img/s line after each epoch, None for no such line
    """
    import time
    import torch
    from .architectures import network_architectures
    from . import evaluation

    lr_epoch_scheduler, lr_iter_scheduler = schedulers
    iter_i = 0
    print('Training...')
    for epoch_i in range(num_epochs):
        if lr_epoch_scheduler is not None:
            lr_epoch_scheduler.step(epoch_i)
        t1 = time.time()
        ramp_val = network_architectures.sigmoid_rampup(epoch_i, rampup) if rampup > 0 else 1.0

        student_net.train()
        if teacher_net is not student_net:
            teacher_net.train()
        if freeze_bn:
            student_net.freeze_batchnorm()
            if teacher_net is not student_net:
                teacher_net.freeze_batchnorm()

        acc = torch.zeros(3, dtype=torch.float64, device=torch_device)    # sup, consistency, conf-rate sums
        n_sup_batches = 0
        n_unsup_batches = 0
        for _ in range(iters_per_epoch):
            if lr_iter_scheduler is not None:
                lr_iter_scheduler.step(iter_i)
            if polls_step_nan and step.nan_detected():
                print('NaN detected; network dead, bailing.')
                return False
            sup_x, sup_y, unsup = make_batch()
            res = step(sup_x, sup_y, unsup, ramp_val=ramp_val)
            n_sup_batches += 1
            n_unsup_batches += accumulate(acc, res, len(unsup), ramp_val, conf_thresh, rampup)
            iter_i += 1

        sup_loss, consistency_loss, conf_rate = epoch_means(acc, n_sup_batches, n_unsup_batches)
        if network_dead(sup_loss, consistency_loss, nan_checks_consistency):
            print('NaN detected; network dead, bailing.')
            return False

        eval_net.eval()
        tgt_iou_eval = evaluation.EvaluatorIoU(n_classes, bin_fill_holes)
        evaluate(tgt_iou_eval)
        if data_parallel:
            tgt_iou_eval.all_reduce()
        tgt_iou = tgt_iou_eval.score()
        tgt_miou = tgt_iou.mean()
        t2 = time.time()
        if rank == 0 or not data_parallel:
            print(epoch_line(epoch_i, t2 - t1, sup_loss, consistency_loss, conf_rate, tgt_miou))
            print('-- {}'.format(', '.join(['{:.3%}'.format(x) for x in tgt_iou])))
            if img_per_s_of is not None:
                batch_size, world = img_per_s_of
                print('-- {:.2f} img/s ({} GPU{})'.format(iters_per_epoch * batch_size * world / max(t2 - t1, 1e-9), world,
                                                          's' if world > 1 else ''))
    return True
