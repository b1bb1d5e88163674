"""
What the four semi-supervised trainers (train_seg_semisup_mask_mt / _vat_mt / _ict / _aug_mt) have in common: the shared blocks
of the reference's option tables, process and device set-up, networks and optimisers, synthetic data, the data set path of
Pascal VOC, CamVid, Cityscapes and ISIC 2017 (pool, index streams, staged evaluation, prediction files, FINAL TEST), and the
epoch loop with its bookkeeping and log lines. A trainer file keeps what is its own: its options, its config / step / batch
construction and how it saves.

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


def open_dataset(synthetic, crop, dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path):
    """The checks of a trainer's data before anything touches the GPU -> None with `--synthetic`, else the reference's data set
    dictionary (datapipe.datasets.load_dataset: any of the five data sets, the splits made on the host exactly as the reference makes
    them).
    Whatever keeps the data set path from starting is a JobNotRun that says so and names `--synthetic`: no log is left behind."""
    import os
    if not synthetic:
        if crop is None:
            raise job_helper.JobNotRun('The data set path stages fixed-size crops on the device: give a --crop_size (whole-image '
                                       'training batches are not built), or run with --synthetic.')
        if int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise job_helper.JobNotRun('The data set path is single-GPU: start one process, or run with --synthetic '
                                       '(which is what serves WORLD_SIZE > 1).')
        from .datapipe import datasets
        from . import settings as settings_mod
        try:
            return datasets.load_dataset(dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path)
        except settings_mod.DataPathError as e:   # no configuration file / no `pascal_voc` path / directory missing
            raise job_helper.JobNotRun('{} -- or run with --synthetic.'.format(e))
    if crop is None:
        raise ValueError('--synthetic needs a --crop_size')
    return None


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


# ------------------------------------------------------------------------------------------------------------------
# the data set path (any source of datapipe.datasets.load_dataset): what the reference's trainers do between `load_dataset` and `FINAL TEST`
def augmenter_options(settings):
    """The `--aug_*` options of a trainer (its `settings`) as the keyword arguments of device_pipeline.DeviceAugmenter."""
    s = settings
    return dict(scale_hung=s['aug_scale_hung'], scale_non_uniform=s['aug_scale_non_uniform'], hflip=s['aug_hflip'],
                vflip=s['aug_vflip'], hvflip=s['aug_hvflip'], strong_colour=s['aug_strong_colour'],
                brightness=s['aug_colour_brightness'], contrast=s['aug_colour_contrast'],
                saturation=s['aug_colour_saturation'], hue=s['aug_colour_hue'], colour_prob=s['aug_colour_prob'],
                greyscale_prob=s['aug_colour_greyscale_prob'], rot_mag=s['aug_rot_mag'], max_scale=s['aug_max_scale'])


class DatasetRun(object):
    """One trainer's run on the data set of `open_dataset`: every image decoded ONCE into an HBM-resident pool
    (resident_pool.py), training crops and padded evaluation batches gathered on the device (device_pipeline.DeviceAugmenter),
    batches drawn from the reference's index streams. The methods are called in the order a reference trainer does these things,
    which is the order of its prints and of its draws from torch's global generator:

        DatasetRun(...)  ->  iters_per_epoch  ->  make_streams  ->  print_sizes_and_start  ->  evaluate / finish
    """

    def __init__(self, ds_dict, torch_device, batch_size):
        import time
        from .resident_pool import ResidentPool
        self.ds_src = ds_dict['ds_src']
        self.val_ndx, self.test_ndx = ds_dict['val_ndx_tgt'], ds_dict['test_ndx_tgt']
        self.sup_ndx, self.unsup_ndx = ds_dict['sup_ndx'], ds_dict['unsup_ndx']
        self.n_classes = self.ds_src.num_classes
        self.batch_size = batch_size
        t0 = time.time()
        self.pool = ResidentPool(self.ds_src, list(self.sup_ndx) + list(self.unsup_ndx) + list(self.val_ndx) +
                                 (list(self.test_ndx) if self.test_ndx is not None else []), torch_device)
        print('Resident pool: {} samples, {:.1f} MB in HBM, decoded in {:.1f}s'.format(
            len(self.pool), self.pool.nbytes() / 1e6, time.time() - t0))

    @classmethod
    def for_evaluation(cls, ds_dict, ndx, net, torch_device, batch_size, dtype):
        """A run that only evaluates `net` over the samples `ndx` (eval_seg): the pool holds nothing else, and the augmenter is
        what make_streams builds (statistics from the network, else the source), with no training crop and no index streams."""
        from .resident_pool import ResidentPool
        from .device_pipeline import DeviceAugmenter
        run = cls.__new__(cls)
        run.ds_src = ds_dict['ds_src']
        run.val_ndx, run.test_ndx = ds_dict['val_ndx_tgt'], ds_dict['test_ndx_tgt']
        run.sup_ndx, run.unsup_ndx = ds_dict['sup_ndx'], ds_dict['unsup_ndx']
        run.n_classes = run.ds_src.num_classes
        run.batch_size = batch_size
        run.pool = ResidentPool(run.ds_src, list(ndx), torch_device)
        mean, std = run.ds_src.get_mean_std()
        mean = net.MEAN if net.MEAN is not None else mean
        std = net.STD if net.STD is not None else std
        run.student_net = net
        run.augment = DeviceAugmenter((1, 1), mean, std, out_dtype=dtype)
        return run

    def iters_per_epoch(self, iters_per_epoch):
        """`--iters_per_epoch -1` is len(unsup_ndx) // batch_size in all four reference trainers."""
        if iters_per_epoch != -1:
            return iters_per_epoch
        if len(self.unsup_ndx) // self.batch_size == 0:
            raise job_helper.JobNotRun('--iters_per_epoch -1 means len(unsup_ndx) // batch_size = {} // {} = 0 iterations per '
                                       'epoch: give --iters_per_epoch or a smaller --batch_size.'.format(
                                           len(self.unsup_ndx), self.batch_size))
        return len(self.unsup_ndx) // self.batch_size

    def make_streams(self, student_net, crop, dtype, settings, n_unsup_streams):
        """The augmenter (statistics from the network, else the source; the reference seeds none of its numpy draws, neither does
        this path) and the RepeatSampler(SubsetRandomSampler) index streams: the supervised one and `n_unsup_streams` (0, 1, or
        the CutMix trainer's 2 that share one sampler) unsupervised ones. -> the augmenter"""
        from .device_pipeline import DeviceAugmenter
        from .datapipe import seg_data
        mean, std = self.ds_src.get_mean_std()
        mean = student_net.MEAN if student_net.MEAN is not None else mean
        std = student_net.STD if student_net.STD is not None else std
        self.student_net = student_net
        self.augment = DeviceAugmenter(crop, mean, std, out_dtype=dtype, **augmenter_options(settings))
        self._streams = [seg_data.repeat_stream(self.sup_ndx, self.batch_size)[0]]
        if n_unsup_streams > 0:
            stream_0, sampler = seg_data.repeat_stream(self.unsup_ndx, self.batch_size)
            self._streams += [stream_0] + [seg_data.IndexStream(sampler, self.batch_size) for _ in range(n_unsup_streams - 1)]
        return self.augment

    def print_sizes_and_start(self, n_sup):
        """The data set size prints, then the iterators in the reference's order: each draws its base seed from torch's global
        generator here. -> [supervised iterator, unsupervised iterators...]"""
        print('len(sup_ndx)={}'.format(len(self.sup_ndx)))
        print('len(unsup_ndx)={}'.format(len(self.unsup_ndx)))
        print('len(val_ndx)={}'.format(len(self.val_ndx)))
        if self.test_ndx is not None:
            print('len(test_ndx)={}'.format(len(self.test_ndx)))
        if n_sup != -1:
            print('sup_ndx={}'.format(self.sup_ndx.tolist()))
        return [iter(st) for st in self._streams]

    def staged_eval(self, eval_net, step, ndx, evaluator=None, preds_dir=None, tta=None, boundary=None, crf=None, surface=None,
                    calibration=None, windows=None, window_batch=None):
        """The reference's evaluation loop over `ndx` in index order: whole images, centred on a padded canvas per batch
        (stage_eval); padding carries label 255 and is ignored. With a `tta.TTA` every batch is evaluated as the vote over its
        views (eval_seg); `step` is read for `align_corners` only. With `boundary` (evaluation.EvaluatorBoundary) the batch's
        prediction -- hole-filled first, on its canvas as `evaluator` fills it, when that fills holes -- is scored against the labels
        with every image's own size;
        the files in `preds_dir` stay the plain prediction. `surface` (evaluation.EvaluatorSurface) is given the map `boundary` is. With `crf` (crf.CRFParams) the batch's views -- one without `tta` -- are
        forwarded as above and the vote is refined against the canvas' bytes inside every image's rectangle (ops.crf_refine); the
        refined prediction is what `evaluator.sample` counts (its hole filling applies to it), what `boundary` and `surface` score and what
        `preds_dir` receives, and the call returns the device-side int64 [pixels, labels the refinement changed] (else None). With
        `calibration` (evaluation.EvaluatorCalibration; not together with `crf`) the batch's views -- one without `tta` -- are forwarded
        as above and the calibration launch takes the place of the vote launch: it scores the confidence of every labelled pixel and
        gives the prediction and the confusion matrix that `evaluator`, `boundary`, `surface` and `preds_dir` then see. With
        `windows` (tta.Windows; not together with `crf` or `calibration`, which read whole views) every view of the batch -- one
        without `tta` -- is covered by overlapping windows on the batch's padded canvas, forwarded in chunks of at most
        `window_batch` windows and stitched by one ops.window_vote launch; `evaluator`, `boundary`, `surface` and `preds_dir` see the
        stitched prediction, and the call returns the number of windows forwarded."""
        import numpy as np
        import torch
        from . import ops
        from .datapipe import seg_data
        crf_total = None
        n_windows = 0
        if windows is not None:
            if crf is not None or calibration is not None:
                raise ValueError('staged_eval: crf and calibration read whole views, not windows')
            from . import tta as tta_mod
            tta = tta if tta is not None else tta_mod.TTA((1.0,), False)
        if calibration is not None:
            if crf is not None:
                raise ValueError('staged_eval: calibration scores the network\'s own distribution, crf refines it into another one')
            from . import tta as tta_mod
            tta = tta if tta is not None else tta_mod.TTA((1.0,), False)
        if crf is not None:
            from . import crf as crf_mod, tta as tta_mod
            crf_views = tta if tta is not None else tta_mod.TTA((1.0,), False)
            crf_total = torch.zeros(2, dtype=torch.int64, device=self.pool.image_buffer.device)
        with torch.no_grad():
            for batch_ndx in seg_data.eval_batches(ndx, self.batch_size):
                ev = self.augment.stage_eval(self.pool, batch_ndx, self.student_net.BLOCK_SIZE)
                want_pred = preds_dir is not None or boundary is not None or surface is not None
                if crf is not None:
                    block = self.student_net.BLOCK_SIZE
                    logits = [l.float() for l in crf_views.forward_views(eval_net, ev['image'], block)]
                    pred, stats = crf_mod.refine_batch(
                        crf, logits, [f for _, f in crf_views.views()], crf_mod.canvas_rgb(self.augment, self.pool, batch_ndx, block),
                        crf_mod.rects_of(ev['offsets'], self.pool.sizes_of(batch_ndx)), self.n_classes, ev['canvas'],
                        step.align_corners)
                    crf_total += stats
                    if evaluator is not None:
                        evaluator.sample(ev['labels'][:, 0], pred, ignore_value=255)
                elif tta is not None:
                    more = {} if calibration is None else dict(calibration=calibration)
                    if windows is not None:
                        more = dict(windows=windows, window_batch=window_batch)
                        n_windows += len(batch_ndx) * tta.window_count(ev['canvas'], self.student_net.BLOCK_SIZE, windows)
                    _, pred = tta.predict(eval_net, ev['image'], ev['canvas'], step.align_corners, labels=ev['labels'],
                                          ignore_index=255, want_pred=want_pred,
                                          block_size=self.student_net.BLOCK_SIZE, evaluator=evaluator, **more)
                else:
                    logits = eval_net.forward_lowres(ev['image'])
                    if evaluator is not None:
                        evaluator.sample_logits(logits, ev['labels'], ev['canvas'], ignore_value=255,
                                                align_corners=step.align_corners)
                    if want_pred:
                        _, pred = ops.argmax_confusion(logits, None, self.n_classes, ev['canvas'],
                                                       align_corners=step.align_corners, want_pred=True)
                if boundary is not None or surface is not None:
                    scored = ops.fill_holes(pred)[0] if getattr(evaluator, 'fill_holes', False) else pred
                    if boundary is not None:
                        boundary.sample(ev['labels'][:, 0], scored, sizes=self.pool.sizes_of(batch_ndx), ignore_value=255)
                    if surface is not None:
                        surface.sample(ev['labels'][:, 0], scored, ignore_value=255)
                if preds_dir is not None:
                    pred = pred.cpu().numpy()
                    for k, sample_ndx in enumerate(batch_ndx):
                        self.ds_src.save_prediction_by_index(preds_dir, pred[k].astype(np.uint32), sample_ndx)
        return crf_total if windows is None else n_windows

    def evaluate_with(self, eval_net, step):
        """-> the `evaluate(evaluator)` of run_epochs over the validation set."""
        return lambda evaluator: self.staged_eval(eval_net, step, self.val_ndx, evaluator)

    def finish(self, eval_net, step, save_preds, submit_config, bin_fill_holes):
        """After the last epoch: prediction files with `--save_preds` (every source inherits
        DataSource.save_prediction_by_index), then the held-out test set and `FINAL TEST` when `--n_val` left one."""
        import os
        from . import evaluation
        out_dir = None
        eval_net.eval()
        if save_preds:
            out_dir = os.path.join(submit_config.run_dir, 'preds')
            os.makedirs(out_dir, exist_ok=True)
            self.staged_eval(eval_net, step, self.val_ndx, None, out_dir)
        if self.test_ndx is not None:
            test_iou_eval = evaluation.EvaluatorIoU(self.n_classes, bin_fill_holes)
            self.staged_eval(eval_net, step, self.test_ndx, test_iou_eval, out_dir)
            test_iou = test_iou_eval.score()
            print('FINAL TEST: mIoU={:.3%}'.format(test_iou.mean()))
            print('-- TEST {}'.format(', '.join(['{:.3%}'.format(x) for x in test_iou])))


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
               nan_checks_consistency, polls_step_nan, rank=0, img_per_s_of=None, after_epoch=None):
    """'Training...' and the epochs: `step(*make_batch(), ramp_val=...)` per iteration with the losses summed on the device,
    then `evaluate(evaluator)` and the epoch's log lines -> False when the network died (said so; the job ends), else True.

      schedulers              (per-epoch, per-iteration) of lr_schedules.make_lr_schedulers
      data_parallel           sum the confusion matrix over the ranks and print on `rank` 0 only; without it every process prints
      nan_checks_consistency  a NaN consistency loss ends the job as a NaN supervised loss does
      polls_step_nan          ask `step.nan_detected()` before every iteration as well
      img_per_s_of            (batch_size, world) to print the img/s line after each epoch, None for no such line
      after_epoch             `after_epoch(epoch_i)` is called behind an epoch's log lines (a trainer's own line), None for nothing
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
            if after_epoch is not None:
                after_epoch(epoch_i)
    return True
