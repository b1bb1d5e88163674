"""
Score a trained model: `python eval_seg.py MODEL.pth --dataset pascal_aug [--subset val|test] [--scales 0.5,0.75,1,1.25,1.5,1.75]
[--flip] [--batch_size 10] [--n_val -1] [--val_seed 131] [--split_path FILE] [--bin_fill_holes] [--save_preds DIR]
[--compute_dtype bf16|fp32] [--boundary_width 3,5,0.02] [--crf [--crf_iters 5] [--crf_radius 5] [--crf_dilation 3] [--crf_bi_w 4]
[--crf_bi_xy 15] [--crf_bi_rgb 13] [--crf_pos_w 3] [--crf_pos_xy 3]] [--surface_dist] [--calibration [--calib_bins 15]
[--calib_thresh 0.5,0.9,0.95,0.97,0.99] [--calib_temperature 1] [--calib_nll_temps LIST] [--calib_out FILE.json]]
[--window H,W [--window_stride H,W] [--window_batch N]]`.

The reference has no such program: it evaluates inside a training run only, at one scale without a flip. MODEL.pth is the whole-module
pickle a trainer writes with `--save_model` (or the reference's own). The data set is opened exactly as the trainers open it
(datapipe.datasets.load_dataset, `./semantic_segmentation.cfg`), so the same `--n_val` / `--val_seed` / `--split_path` give the same
validation and test sets; only the chosen subset is decoded into the HBM-resident pool. Every batch goes through
trainer_common.DatasetRun.staged_eval: whole images on a padded canvas, one forward pass per view (tta.TTA), one launch of the vote
kernel (csrc/tta.hip). The output is the trainers': `VAL mIoU=...` (or `TEST mIoU=...`) and the `-- ` per-class line; with the defaults
(`--scales 1`, no `--flip`) the numbers are bit for bit those of the trainer's last evaluation of that model.

`--boundary_width SPEC` (off by default) adds the contour scores of evaluation.EvaluatorBoundary for up to four band widths, an integer
being pixels and a number in (0, 1) a ratio of each image's own diagonal: after the two lines above, per width in the order given,
`VAL BIoU@<w>=...` (Boundary IoU, Cheng et al. 2021) with its per-class line `-- BIoU@<w> ...`, then `VAL trimap@<w>=...` (the IoU over
the pixels within <w> of a ground-truth boundary) with `-- trimap@<w> ...`. The prediction scored is the one the mIoU line scores
(the vote, hole-filled with `--bin_fill_holes`); the first two lines do not change.

`--crf` (off by default) refines every batch's vote against its image before anything is counted: crf.py's truncated, dilated-window
form of the fully connected CRF the DeepLab papers report their numbers after (csrc/crf.hip). The refined prediction is what the mIoU
line, `--bin_fill_holes`, `--boundary_width` and `--save_preds` then see, and after the two lines above one more says what it did:
`-- CRF changed x.xxx% of the pixels`. The `--crf_*` values are crf.CRFParams'; their defaults are not tuned. Without `--crf` every
printed line and every saved file is what it was.

`--surface_dist` (off by default) adds the surface distances of evaluation.EvaluatorSurface, in pixels of the evaluated image, after
every line above: `VAL HD95=...` with its per-class line `-- HD95 ...`, then `VAL ASSD=...` / `-- ASSD ...` and `VAL HD=...` / `-- HD ...`
(the Hausdorff distance, its 95th percentile and the average symmetric surface distance in MedPy's convention; csrc/surface.hip), and
`-- surface pairs ... (one-sided ...)`. A class is scored in the images in which both the labels and the prediction hold it; its
number is the mean over those images, `-` when there is none, and the headline the mean over the classes that have one. The images
in which only one of the two holds the class are counted as one-sided. The prediction scored is the one `--boundary_width` scores.
Without the option every printed line and every saved file is what it was.

`--calibration` (off by default) scores the confidence the trainers compare with `--conf_thresh` (evaluation.EvaluatorCalibration,
csrc/calib.hip: one launch per batch in the place of the vote launch), after every line above: `VAL ECE=...` with its per-class line
`-- ECE ...` (by predicted class, `-` for a class that is never predicted), `-- MCE=... NLL=... Brier=...`, one `-- bin [lo,hi) n=...
acc=... conf=...` row per equal-width bin, then per threshold `VAL pseudo@<t> pass=...% acc=...%` with `-- pseudo@<t> acc ...` (by
predicted class) and `-- pseudo@<t> recall ...` (by true class: the share of its pixels that receive a correct pseudo-label), and with
`--calib_nll_temps` the line `-- NLL@T ...; lowest at T=...`. `--calib_temperature T` divides the logits by T before the softmax; with
two or more views the vote itself is then taken at T and one line says so. The tables score the network's own distribution:
`--bin_fill_holes` does not touch them, and `--crf` is refused beside them. With T = 1 the mIoU lines are bit for bit what they are
without the option. `--calib_out FILE.json` writes the integer tables and every derived score.

`--window H,W` (or one integer; off by default) evaluates by sliding window, as the semi-supervised segmentation papers report
Cityscapes: every view of a batch is covered by overlapping windows of that size (tta.Windows, include/cutmixseg.h states the grid), the
network sees the windows -- `--window_batch N` at a time, by default `--batch_size` -- and one launch stitches them: a pixel's score is
the mean softmax probability of the windows that cover it, summed over the views (csrc/window.hip). `--window_stride H,W` (or one
integer) defaults to ceil(2 * window / 3) and lies in [ceil(window / 4), window]; the window is a multiple of the network's block size.
After the two lines above one more says what was done: `-- sliding window 512x1024 stride 342x683: 4500 windows over 500 images`.
`--bin_fill_holes`, `--boundary_width`, `--surface_dist` and `--save_preds` see the stitched prediction; `--crf` and `--calibration`
read whole views and are refused beside it. The windows tile the batch's padded canvas: with images of one size, or `--batch_size 1`,
an image's prediction does not depend on its batch; with images of several sizes and a larger batch it can. Without `--window` every
printed line and every saved file is what it was.

What keeps the program from starting is said before the GPU is touched: a bad `--window*` value or one without `--window`, `--window`
with `--crf` or `--calibration`, a window that is not a multiple of the network's block size, a bad `--calib_*` value or one without `--calibration`,
`--calibration` with `--crf`, a model file that does not load, a data set that is not
configured, `--subset test` without a held-out set, `--bin_fill_holes` on more than two classes, a model of another class count, bad
`--scales`, a bad `--boundary_width`, a bad `--crf_*` value or one without `--crf`, more than one process.
"""
import os

import click


class EvalNotRun(click.ClickException):
    """Why eval_seg does not start; click prints it and exits non-zero."""


def model_num_classes(net):
    """The class count of a loaded network: its `num_classes`, else the width of its last convolution."""
    import torch
    n = getattr(net, 'num_classes', None)
    if n is not None:
        return int(n)
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    if not convs:
        raise EvalNotRun('the model has no convolution to read a class count from')
    return int(convs[-1].out_channels)


def boundary_spec(text):
    """--boundary_width as [(label, width)] in the order given, the label being the entry as it was typed; None without the option"""
    if text is None:
        return None
    from . import evaluation
    try:
        widths = evaluation.parse_boundary_widths(text)
    except ValueError as e:
        raise EvalNotRun('--boundary_width: {}'.format(e))
    return list(zip([p.strip() for p in text.split(',')], widths))


CRF_OPTIONS = ('crf_iters', 'crf_radius', 'crf_dilation', 'crf_bi_w', 'crf_bi_xy', 'crf_bi_rgb', 'crf_pos_w', 'crf_pos_xy')


def crf_spec(crf, **options):
    """--crf and the --crf_* values as they were typed (None where not given) -> crf.CRFParams, or None without --crf"""
    from . import crf as crf_mod
    try:
        return crf_mod.CRFParams.from_options(bool(crf), **options)
    except ValueError as e:
        raise EvalNotRun(str(e))


CALIB_OPTIONS = ('calib_bins', 'calib_thresh', 'calib_temperature', 'calib_nll_temps', 'calib_out')


def calibration_spec(calibration, calib_bins=None, calib_thresh=None, calib_temperature=None, calib_nll_temps=None, calib_out=None,
                     crf=None):
    """--calibration and the --calib_* values as they were typed (None where not given) -> dict(n_bins, thresholds, labels,
    temperature, nll_temperatures, out) for evaluation.EvaluatorCalibration, or None without --calibration. No GPU."""
    given = dict(calib_bins=calib_bins, calib_thresh=calib_thresh, calib_temperature=calib_temperature,
                 calib_nll_temps=calib_nll_temps, calib_out=calib_out)
    if not calibration:
        for k, v in given.items():
            if v is not None:
                raise EvalNotRun('--{} is given without --calibration'.format(k))
        return None
    if crf:
        raise EvalNotRun('--calibration scores the network\'s own softmax confidence; --crf replaces it with another distribution: '
                         'give one of the two')
    from . import evaluation
    try:
        n_bins = int(str(calib_bins).strip()) if calib_bins is not None else 15
    except ValueError:
        raise EvalNotRun('--calib_bins {!r}: an integer in 1..48 is needed'.format(calib_bins))
    thresh_text = '0.5,0.9,0.95,0.97,0.99' if calib_thresh is None else str(calib_thresh)
    try:
        thresholds = evaluation.parse_calibration_thresholds(thresh_text)
    except ValueError as e:
        raise EvalNotRun('--calib_thresh: {}'.format(e))
    try:
        temperature = evaluation.parse_calibration_temperatures('1' if calib_temperature is None else calib_temperature)
        if len(temperature) != 1:
            raise ValueError('one number is needed, got {!r}'.format(calib_temperature))
    except ValueError as e:
        raise EvalNotRun('--calib_temperature: {}'.format(e))
    try:
        more = evaluation.parse_calibration_temperatures('' if calib_nll_temps is None else calib_nll_temps)
        if len(more) > evaluation.CALIB_MAX_TEMPS - 1:
            raise ValueError('{} temperatures, at most {} are taken'.format(len(more), evaluation.CALIB_MAX_TEMPS - 1))
    except ValueError as e:
        raise EvalNotRun('--calib_nll_temps: {}'.format(e))
    try:
        evaluation.calibration_edges(n_bins, thresholds)
    except ValueError as e:
        raise EvalNotRun('--calib_bins / --calib_thresh: {}'.format(e))
    labels = [p.strip() for p in thresh_text.split(',')] if thresholds else []
    return dict(n_bins=n_bins, thresholds=thresholds, labels=labels, temperature=temperature[0], nll_temperatures=more, out=calib_out)


def window_spec(window, window_stride=None, window_batch=None, crf=None, calibration=None):
    """--window, --window_stride and --window_batch as they were typed (None where not given; pairs and integers are taken too) ->
    (tta.Windows, window_batch or None), or None without --window. No GPU, no torch."""
    from . import tta as tta_mod
    if window is None:
        for name, v in (('window_stride', window_stride), ('window_batch', window_batch)):
            if v is not None:
                raise EvalNotRun('--{} is given without --window'.format(name))
        return None
    if crf is not None and crf is not False:
        raise EvalNotRun('--window with --crf: the CRF launch reads whole views, not windows; give one of the two')
    if calibration is not None and calibration is not False:
        raise EvalNotRun('--window with --calibration: the calibration launch reads whole views, not windows; give one of the two')

    def pair(v, what):
        return tta_mod.parse_window(v, what) if isinstance(v, str) else v
    try:
        windows = tta_mod.Windows(pair(window, '--window'), None if window_stride is None else pair(window_stride, '--window_stride'))
    except ValueError as e:
        raise EvalNotRun(str(e) if str(e).startswith('--window') else '--window / --window_stride: {}'.format(e))
    if window_batch is not None:
        try:
            window_batch = int(str(window_batch).strip())
        except ValueError:
            raise EvalNotRun('--window_batch {!r}: an integer of at least 1 is needed'.format(window_batch))
        if window_batch < 1:
            raise EvalNotRun('--window_batch must be at least 1, got {}'.format(window_batch))
    return windows, window_batch


def check_window_block(windows, block_size):
    """a window that is not a multiple of the network's block size does not start"""
    try:
        windows.check_block(block_size)
    except ValueError as e:
        raise EvalNotRun('--window: {}'.format(e))


def prepare(model_path, dataset, subset, scales, flip, n_val, val_seed, split_path, bin_fill_holes, boundary_width=None,
            calibration=None, crf=None, windows=None):
    """Everything that can refuse, on the host -> (tta, net on the CPU, ds_dict, ndx). `calibration`: calibration_spec's dict, or
    (flag, dict of the --calib_* values as typed), checked here. `windows`: a tta.Windows, held to the loaded network's block size."""
    from . import tta as tta_mod
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise EvalNotRun('eval_seg runs on one GPU: start one process (WORLD_SIZE={})'.format(os.environ['WORLD_SIZE']))
    boundary_spec(boundary_width)
    if isinstance(calibration, tuple):
        calibration_spec(calibration[0], crf=crf, **calibration[1])
    elif calibration is not None and crf:
        calibration_spec(True, crf=crf)
    try:
        tta = tta_mod.TTA(tta_mod.parse_scales(scales), flip)
    except ValueError as e:
        raise EvalNotRun(str(e))

    from . import checkpoint, job_helper, settings
    import torch
    try:
        net = checkpoint.load_model(model_path)
    except Exception as e:           # whatever the file is instead of a module pickle
        raise EvalNotRun('the model file {} does not load: {}: {}'.format(model_path, type(e).__name__, e))
    if not isinstance(net, torch.nn.Module) or not hasattr(net, 'forward_lowres'):
        raise EvalNotRun('the model file {} holds a {}, not a whole network of this project (a trainer writes one with '
                         '--save_model)'.format(model_path, type(net).__name__))
    if windows is not None:
        check_window_block(windows, getattr(net, 'BLOCK_SIZE', (1, 1)))

    from .datapipe import datasets
    try:
        ds_dict = datasets.load_dataset(dataset, n_val, val_seed, -1, -1, 12345, split_path)
    except (settings.DataPathError, job_helper.JobNotRun) as e:
        raise EvalNotRun(str(e))
    ndx = ds_dict['val_ndx_tgt'] if subset == 'val' else ds_dict['test_ndx_tgt']
    if ndx is None:
        raise EvalNotRun('--subset test: --n_val {} leaves no test set (with --n_val > 0 the official validation list becomes '
                         'the test set)'.format(n_val))
    if len(ndx) == 0:
        raise EvalNotRun('--subset {}: the set is empty'.format(subset))
    n_classes = ds_dict['ds_src'].num_classes
    if bin_fill_holes and n_classes != 2:
        raise EvalNotRun('--bin_fill_holes: binary hole filling needs a binary (2-class) data set, {} has {} classes'.format(
            dataset, n_classes))
    if model_num_classes(net) != n_classes:
        raise EvalNotRun('the model predicts {} classes, the data set {} has {}'.format(model_num_classes(net), dataset, n_classes))
    return tta, net, ds_dict, ndx


def evaluate(model_path, dataset, subset='val', scales='1', flip=False, batch_size=10, n_val=-1, val_seed=131, split_path=None,
             bin_fill_holes=False, save_preds=None, compute_dtype='bf16', boundary_width=None, crf=None, surface_dist=False,
             calibration=None, window=None, window_stride=None, window_batch=None):
    """-> the per-class IoU (numpy); prints the trainers' lines, with `crf` (crf.CRFParams) what the refinement changed, with
    `boundary_width` the contour scores after them, with `surface_dist` the surface distances after those, and with `calibration`
    (calibration_spec's dict; True for the defaults) the calibration report after everything else. `window` / `window_stride`
    (text as typed, or pairs) and `window_batch`: sliding-window evaluation (window_spec), its line after the two mIoU lines."""
    if crf is not None and not hasattr(crf, 'as_dict'):
        raise EvalNotRun('crf must be a crf.CRFParams, got {!r}'.format(crf))
    if calibration is True:
        calibration = calibration_spec(True, crf=crf)
    elif calibration is not None and not isinstance(calibration, dict):
        raise EvalNotRun('calibration must be True or the dict of calibration_spec, got {!r}'.format(calibration))
    win = window_spec(window, window_stride, window_batch, crf=crf, calibration=calibration)
    tta, net, ds_dict, ndx = prepare(model_path, dataset, subset, scales, flip, n_val, val_seed, split_path, bin_fill_holes,
                                     boundary_width, calibration, crf, None if win is None else win[0])
    spec = boundary_spec(boundary_width)

    import types
    import torch
    from . import evaluation, trainer_common as tc
    if not torch.cuda.is_available():
        raise RuntimeError('eval_seg needs a GPU; there is no CPU fallback')
    torch.cuda.set_device(0)
    torch_device = torch.device('cuda', 0)
    dtype = torch.bfloat16 if compute_dtype == 'bf16' else torch.float32
    net = net.to(torch_device)
    net.compute_dtype = dtype
    for p in net.parameters():
        p.requires_grad = False
    net.eval()

    run = tc.DatasetRun.for_evaluation(ds_dict, ndx, net, torch_device, batch_size, dtype)
    step = types.SimpleNamespace(align_corners=getattr(net, 'upsample_align_corners', True))
    if save_preds is not None:
        os.makedirs(save_preds, exist_ok=True)
    iou_eval = evaluation.EvaluatorIoU(run.n_classes, bin_fill_holes)
    more = {} if crf is None else dict(crf=crf)
    bd_eval = None
    if spec is not None:
        try:
            bd_eval = evaluation.EvaluatorBoundary(run.n_classes, [w for _, w in spec])
        except ValueError as e:
            raise EvalNotRun('--boundary_width: {}'.format(e))
        more['boundary'] = bd_eval
    sf_eval = None
    if surface_dist:
        sf_eval = more['surface'] = evaluation.EvaluatorSurface(run.n_classes)
    cal_eval = None
    if calibration is not None:
        cal_eval = more['calibration'] = evaluation.EvaluatorCalibration(
            run.n_classes, calibration['n_bins'], calibration['thresholds'], calibration['temperature'], calibration['nll_temperatures'])
    if win is not None:
        more.update(windows=win[0], window_batch=win[1] if win[1] is not None else batch_size)
    crf_stats = run.staged_eval(net, step, ndx, iou_eval, save_preds, tta=tta, **more)
    iou = iou_eval.score()
    prefix = 'VAL' if subset == 'val' else 'TEST'
    print('{} mIoU={:.3%}'.format(prefix, iou.mean()))
    print('-- {}'.format(', '.join(['{:.3%}'.format(x) for x in iou])))
    if win is not None:
        print('-- sliding window {}x{} stride {}x{}: {} windows over {} images'.format(
            win[0].window[0], win[0].window[1], win[0].stride[0], win[0].stride[1], int(crf_stats), len(ndx)))
    if crf is not None:
        pixels, changed = (int(v) for v in crf_stats.cpu().tolist())
        print('-- CRF changed {:.3%} of the pixels'.format(changed / max(pixels, 1)))
    if spec is not None:
        for (label, _), b_iou, t_iou in zip(spec, bd_eval.boundary_iou(), bd_eval.trimap_iou()):
            for name, score in (('BIoU', b_iou), ('trimap', t_iou)):
                print('{} {}@{}={:.3%}'.format(prefix, name, label, score.mean()))
                print('-- {}@{} {}'.format(name, label, ', '.join(['{:.3%}'.format(x) for x in score])))
    if sf_eval is not None:
        for name, score in (('HD95', sf_eval.hd95()), ('ASSD', sf_eval.assd()), ('HD', sf_eval.hd())):
            print('{} {}={:.3f}'.format(prefix, name, sf_eval.headline(score)))
            print('-- {} {}'.format(name, ', '.join(['-' if x != x else '{:.3f}'.format(x) for x in score])))
        scored, one_sided = sf_eval.pairs()
        print('-- surface pairs {} (one-sided {})'.format(', '.join(str(int(x)) for x in scored),
                                                          ', '.join(str(int(x)) for x in one_sided)))
    if cal_eval is not None:
        for line in calibration_lines(prefix, cal_eval, calibration['labels'], len(tta.views())):
            print(line)
        if calibration.get('out'):
            import json
            with open(calibration['out'], 'w') as f:
                json.dump(cal_eval.as_dict(), f)
    return iou


def calibration_lines(prefix, cal, labels, n_views=1):
    """The printed calibration report of an evaluation.EvaluatorCalibration; `labels`: the thresholds as they were typed."""
    def pct(x, digits=3):
        return '-' if x != x else '{:.{}%}'.format(x, digits)
    lines = []
    if cal.temperature != 1.0:
        lines.append('-- calibration at T={:g}{}'.format(
            cal.temperature, ': the vote over the {} views is taken at T'.format(n_views) if n_views >= 2 else ''))
    lines.append('{} ECE={}'.format(prefix, pct(cal.ece())))
    lines.append('-- ECE {}'.format(', '.join(pct(x) for x in cal.ece_per_class())))
    nll = cal.nll()
    lines.append('-- MCE={} NLL={:.4f} Brier={:.4f}'.format(pct(cal.mce()), nll[0], cal.brier()))
    for row in cal.reliability():
        lines.append('-- bin [{:.3f},{:.3f}) n={} acc={} conf={}'.format(row['lo'], row['hi'], row['n'], pct(row['acc']), pct(row['conf'])))
    for label, rep in zip(labels, cal.threshold_report()):
        lines.append('{} pseudo@{} pass={} acc={}'.format(prefix, label, pct(rep['pass_rate']), pct(rep['acc'])))
        lines.append('-- pseudo@{} acc {}'.format(label, ', '.join(pct(x) for x in rep['acc_per_class'])))
        lines.append('-- pseudo@{} recall {}'.format(label, ', '.join(pct(x) for x in rep['recall_per_class'])))
    if len(cal.temperatures) > 1:
        best = min(range(len(nll)), key=lambda i: (nll[i] != nll[i], nll[i]))
        lines.append('-- NLL@T {}; lowest at T={:g}'.format(
            ', '.join('{:g}={:.4f}'.format(t, v) for t, v in zip(cal.temperatures, nll)), cal.temperatures[best]))
    return lines


@click.command()
@click.argument('model_path', type=click.Path())
@click.option('--dataset', type=click.Choice(['camvid', 'cityscapes', 'pascal', 'pascal_aug', 'isic2017']), default='pascal_aug')
@click.option('--subset', type=click.Choice(['val', 'test']), default='val')
@click.option('--scales', type=str, default='1')
@click.option('--flip', is_flag=True, default=False)
@click.option('--batch_size', type=int, default=10)
@click.option('--n_val', type=int, default=-1)
@click.option('--val_seed', type=int, default=131)
@click.option('--split_path', type=click.Path(readable=True, exists=True))
@click.option('--bin_fill_holes', is_flag=True, default=False)
@click.option('--save_preds', type=click.Path(file_okay=False), default=None)
@click.option('--compute_dtype', type=click.Choice(['bf16', 'fp32']), default='bf16')
@click.option('--boundary_width', type=str, default=None)
@click.option('--crf', is_flag=True, default=False)
@click.option('--crf_iters', type=str, default=None, help='5')
@click.option('--crf_radius', type=str, default=None, help='5')
@click.option('--crf_dilation', type=str, default=None, help='3')
@click.option('--crf_bi_w', type=str, default=None, help='4')
@click.option('--crf_bi_xy', type=str, default=None, help='15')
@click.option('--crf_bi_rgb', type=str, default=None, help='13')
@click.option('--crf_pos_w', type=str, default=None, help='3')
@click.option('--crf_pos_xy', type=str, default=None, help='3')
@click.option('--surface_dist', is_flag=True, default=False)
@click.option('--calibration', is_flag=True, default=False)
@click.option('--calib_bins', type=str, default=None, help='15')
@click.option('--calib_thresh', type=str, default=None, help='0.5,0.9,0.95,0.97,0.99')
@click.option('--calib_temperature', type=str, default=None, help='1')
@click.option('--calib_nll_temps', type=str, default=None, help='up to seven more temperatures for the NLL line')
@click.option('--calib_out', type=click.Path(dir_okay=False), default=None)
@click.option('--window', type=str, default=None, help='H,W or one integer: sliding-window evaluation')
@click.option('--window_stride', type=str, default=None, help='ceil(2 * window / 3)')
@click.option('--window_batch', type=str, default=None, help='windows per forward pass; --batch_size')
def experiment(model_path, dataset, subset, scales, flip, batch_size, n_val, val_seed, split_path, bin_fill_holes, save_preds,
               compute_dtype, boundary_width, crf, surface_dist, calibration, **options):
    if batch_size < 1:
        raise EvalNotRun('--batch_size must be at least 1')
    calib_options = {k: options.pop(k) for k in CALIB_OPTIONS}
    window_options = {k: options.pop(k) for k in ('window', 'window_stride', 'window_batch')}
    window_spec(crf=crf, calibration=calibration, **window_options)      # a malformed --window* value, or --window beside --crf
    boundary_spec(boundary_width)                  # a malformed one is said before the model file is even opened
    calib = calibration_spec(calibration, crf=crf, **calib_options)      # ... and a --calib_* value, or --calibration beside --crf
    params = crf_spec(crf, **options)              # ... and so is a malformed --crf_* value, or one without --crf
    evaluate(model_path, dataset, subset, scales, flip, batch_size, n_val, val_seed, split_path, bin_fill_holes, save_preds,
             compute_dtype, boundary_width, params, surface_dist, calib, **window_options)


if __name__ == '__main__':
    experiment()
