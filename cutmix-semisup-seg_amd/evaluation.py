"""
Mirror of the reference's evaluation.py (fast_cm, per_class_i_and_u_cm, EvaluatorIoU) backed by the confusion-matrix
kernels of csrc/eval.hip.

The reference loops over classes in numpy on the host (evaluation.py:24-33; 0.28 s per 321x321 image at 21 classes).
Here truth / prediction maps are histogrammed on the GPU into one C x C int64 matrix; intersection and union follow
from it exactly: I = diag(cm), U = rowsum + colsum - diag (integer identity).
`EvaluatorIoU.sample_logits` is the fused path used by the trainer: bilinear upsample + argmax + histogram straight
from the network's low-resolution logits, nothing full-resolution ever leaves the device. With `fill_holes` (binary
configurations) the argmax map is hole-filled on the device as well (csrc/fillholes.hip), fused with the histogram.
"""
import math

import numpy as np
import torch

from . import ops


def _to_u8_cuda(a, device, what):
    if torch.is_tensor(a):
        t = a
    else:
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError('{} values must lie in [0, 255]'.format(what))
        t = t.to(torch.uint8)
    return t.to(device, non_blocking=True).contiguous()


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('evaluation runs on the GPU only; no CUDA/HIP device available')
    return torch.device('cuda', torch.cuda.current_device())


def fast_cm(tru, pred, num_classes):
    """Confusion matrix (row = true class, column = predicted class), evaluation.py:6-16."""
    dev = _device()
    cm = ops.confusion(_to_u8_cuda(tru, dev, 'tru'), _to_u8_cuda(pred, dev, 'pred'), num_classes)
    return cm.cpu().numpy()


def per_class_i_and_u_cm(pred, tru, num_classes, ignore_value=None):
    """-> (intersection (C,), union (C,), cm (C,C)) as integer numpy arrays, evaluation.py:18-37."""
    dev = _device()
    cm = ops.confusion(_to_u8_cuda(tru, dev, 'tru'), _to_u8_cuda(pred, dev, 'pred'), num_classes,
                       ignore_index=ignore_value).cpu().numpy()
    diag = np.diag(cm)
    return diag.copy(), cm.sum(axis=0) + cm.sum(axis=1) - diag, cm


def parse_boundary_widths(text):
    """'3,5,0.02' -> [3, 5, 0.02]: an integer in 1..254 is a band width in pixels, a number in (0, 1) a ratio of the image's own
    diagonal (Boundary IoU's default is 0.02). One to four entries; anything else raises ValueError."""
    if not isinstance(text, str):
        raise ValueError('boundary widths must be given as text such as "3,5,0.02", got {!r}'.format(text))
    parts = [p.strip() for p in text.split(',')]
    if not 1 <= len(parts) <= 4:
        raise ValueError('boundary widths: one to four comma-separated entries, got {!r}'.format(text))
    out = []
    for p in parts:
        try:
            v = int(p)
        except ValueError:
            try:
                v = float(p)
            except ValueError:
                raise ValueError('boundary widths: {!r} is neither a width in pixels nor a ratio of the diagonal'.format(p))
            if not 0.0 < v < 1.0:             # NaN included
                raise ValueError('boundary widths: a ratio of the diagonal lies in (0, 1), got {!r}'.format(p))
        else:
            if not 1 <= v <= 254:
                raise ValueError('boundary widths: a width in pixels lies in 1..254, got {!r}'.format(p))
        out.append(v)
    return out


def boundary_width_px(spec, size):
    """One entry of a widths specification in pixels for an image of `size` (h, w): the integer itself, or
    max(1, round(ratio * diagonal)) (at most 254, the widest band the kernel tells apart)."""
    if isinstance(spec, (int, np.integer)):
        return int(spec)
    h, w = size
    return min(254, max(1, int(round(float(spec) * np.sqrt(float(h * h + w * w))))))


class EvaluatorBoundary(object):
    """Boundary IoU (Cheng et al., CVPR 2021) and trimap IoU over the samples it is given, for up to four band widths at once
    (`widths_spec`: what parse_boundary_widths returns, or its text). Both follow exactly from two integer matrices per width that
    ops.boundary_confusion accumulates on the device: `bcm` (K,C+1,C+1) and `tcm` (K,C,C)."""

    def __init__(self, num_classes, widths_spec):
        if isinstance(widths_spec, str):
            widths_spec = parse_boundary_widths(widths_spec)
        widths_spec = list(widths_spec)
        if not 1 <= len(widths_spec) <= 4:
            raise ValueError('EvaluatorBoundary: one to four widths, got {}'.format(len(widths_spec)))
        for v in widths_spec:
            ok = 1 <= v <= 254 if isinstance(v, (int, np.integer)) else (isinstance(v, float) and 0.0 < v < 1.0)
            if not ok:
                raise ValueError('EvaluatorBoundary: a width is an integer in 1..254 or a ratio in (0, 1), got {!r}'.format(v))
        if not 1 <= int(num_classes) <= 64:
            raise ValueError('EvaluatorBoundary: 1 <= num_classes <= 64, got {}'.format(num_classes))
        self.num_classes = int(num_classes)
        self.widths_spec = widths_spec
        self._bcm_dev = self._tcm_dev = None

    def _matrices(self):
        if self._bcm_dev is None:
            k, c, dev = len(self.widths_spec), self.num_classes, _device()
            self._bcm_dev = torch.zeros((k, c + 1, c + 1), dtype=torch.int64, device=dev)
            self._tcm_dev = torch.zeros((k, c, c), dtype=torch.int64, device=dev)
        return self._bcm_dev, self._tcm_dev

    def sample(self, truth, prediction, sizes=None, ignore_value=255):
        """Accumulate one (H,W) or batched (N,H,W) pair of integer maps. `sizes`: the (h, w) of every image before padding, which
        a width given as a ratio of the diagonal refers to; without it the map's own size. The counts of an image do not depend on
        the padding round it (label `ignore_value`)."""
        dev = _device()
        truth = _to_u8_cuda(truth, dev, 'truth')
        prediction = _to_u8_cuda(prediction, dev, 'prediction')
        n = int(truth.shape[0]) if truth.dim() == 3 else 1
        if sizes is None:
            sizes = [tuple(int(v) for v in truth.shape[-2:])] * n
        if len(sizes) != n:
            raise ValueError('EvaluatorBoundary.sample: {} sizes for {} maps'.format(len(sizes), n))
        widths = np.array([[boundary_width_px(v, s) for v in self.widths_spec] for s in sizes], dtype=np.int32)
        bcm, tcm = self._matrices()
        ops.boundary_confusion(truth, prediction, self.num_classes, widths, ignore_index=ignore_value, bcm=bcm, tcm=tcm)

    @property
    def bcm(self):
        return self._matrices()[0].cpu().numpy()

    @property
    def tcm(self):
        return self._matrices()[1].cpu().numpy()

    def boundary_iou(self):
        """-> (K, C): bcm[c,c] / max(row c + column c - bcm[c,c], 1), the sums over all C + 1 entries"""
        m = self.bcm
        c = self.num_classes
        diag = np.diagonal(m, axis1=1, axis2=2)[:, :c]
        union = m.sum(axis=2)[:, :c] + m.sum(axis=1)[:, :c] - diag
        return diag.astype(float) / np.maximum(union.astype(float), 1.0)

    def trimap_iou(self):
        """-> (K, C): the IoU over the pixels within the width of a ground-truth boundary"""
        m = self.tcm
        diag = np.diagonal(m, axis1=1, axis2=2)
        union = m.sum(axis=2) + m.sum(axis=1) - diag
        return diag.astype(float) / np.maximum(union.astype(float), 1.0)


class EvaluatorSurface(object):
    """The Hausdorff distance (HD), its 95th percentile (HD95) and the average symmetric surface distance (ASSD), in pixels, per class:
    the mean over the images in which both the truth and the prediction hold the class (MedPy's hd / hd95 / assd with connectivity 1,
    as the Medical Segmentation Decathlon reports them). An image in which only one of the two holds the class is counted as one-sided
    and not scored: HD is undefined there. ops.surface_distances leaves exact integers and two fp64 sums per image and class on the
    device; they come to the host once, when a score is asked for."""

    def __init__(self, num_classes):
        if not 1 <= int(num_classes) <= 64:
            raise ValueError('EvaluatorSurface: 1 <= num_classes <= 64, got {}'.format(num_classes))
        self.num_classes = int(num_classes)
        self._stats, self._sums = [], []
        self._done = None

    def sample(self, truth, prediction, ignore_value=255):
        """Score one (H,W) or batched (N,H,W) pair of integer maps. An image's numbers do not depend on the padding round it
        (label `ignore_value`)."""
        dev = _device()
        stats, sums, _ = ops.surface_distances(_to_u8_cuda(truth, dev, 'truth'), _to_u8_cuda(prediction, dev, 'prediction'),
                                               self.num_classes, ignore_index=ignore_value)
        self._stats.append(stats)
        self._sums.append(sums)
        self._done = None

    def _finish(self):
        if self._done is None:
            c = self.num_classes
            if self._stats:
                stats, sums = torch.cat(self._stats).cpu().numpy(), torch.cat(self._sums).cpu().numpy()     # one transfer each
            else:
                stats, sums = np.zeros((0, c, 6), dtype=np.int64), np.zeros((0, c, 2))
            tot = np.zeros((3, c))
            scored, one_sided = np.zeros(c, dtype=np.int64), np.zeros(c, dtype=np.int64)
            for st, sm in zip(stats.tolist(), sums.tolist()):
                for k in range(c):
                    n_p, n_t, max_p, max_t, lo, hi = st[k]
                    if n_p > 0 and n_t > 0:
                        r = (19 * (n_p + n_t - 1)) % 20
                        scored[k] += 1
                        tot[0, k] += math.sqrt(max(max_p, max_t))
                        tot[1, k] += math.sqrt(lo) + (r / 20.0) * (math.sqrt(hi) - math.sqrt(lo))
                        tot[2, k] += 0.5 * (sm[k][0] / n_p + sm[k][1] / n_t)
                    elif n_p > 0 or n_t > 0:
                        one_sided[k] += 1
            with np.errstate(invalid='ignore', divide='ignore'):
                mean = np.where(scored > 0, tot / np.maximum(scored, 1), np.nan)
            self._done = dict(hd=mean[0], hd95=mean[1], assd=mean[2], scored=scored, one_sided=one_sided)
        return self._done

    def hd(self):
        """-> (C,) float64, NaN for a class no image was scored for"""
        return self._finish()['hd'].copy()

    def hd95(self):
        return self._finish()['hd95'].copy()

    def assd(self):
        return self._finish()['assd'].copy()

    def pairs(self):
        """-> the (C,) int64 arrays (scored, one_sided): images per class"""
        done = self._finish()
        return done['scored'].copy(), done['one_sided'].copy()

    @staticmethod
    def headline(score):
        """the mean over the classes that were scored at all (NaN when none was)"""
        ok = ~np.isnan(score)
        return float(score[ok].mean()) if ok.any() else float('nan')


class EvaluatorIoU(object):
    def __init__(self, num_classes, fill_holes=False):
        if fill_holes:
            if num_classes != 2:
                raise ValueError('num_classes must be 2 if fill_holes is True')
        self.num_classes = num_classes
        self.fill_holes = fill_holes
        self._cm_dev = None

    def _cm(self):
        if self._cm_dev is None:
            self._cm_dev = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=_device())
        return self._cm_dev

    def sample(self, truth, prediction, ignore_value=None):
        """Accumulate one (H,W) [or batched (N,H,W)] pair of integer maps (numpy or torch)."""
        dev = _device()
        truth = _to_u8_cuda(truth, dev, 'truth')
        prediction = _to_u8_cuda(prediction, dev, 'prediction')
        if self.fill_holes:
            # binary post-processing (the reference's scipy binary_fill_holes, evaluation.py:53-55) runs on the device, fused with
            # the histogram: csrc/fillholes.hip. A 2-D pair is one image, an (N,H,W) pair N images filled independently.
            ops.fill_holes(prediction, truth=truth, ignore_index=ignore_value, cm=self._cm())
            return
        ops.confusion(truth, prediction, self.num_classes, ignore_index=ignore_value, cm=self._cm())

    def sample_logits(self, logits, truth, out_size=None, ignore_value=255, align_corners=True):
        """Fused: logits (N,C,h,w) CUDA [low-res or full-res], truth (N,H,W)/(N,1,H,W) uint8/int64 CUDA."""
        if self.fill_holes:
            _, pred = ops.argmax_confusion(logits, None, self.num_classes, out_size or truth.shape[-2:],
                                           align_corners=align_corners, want_pred=True)
            t = truth[:, 0] if truth.dim() == 4 else truth
            # the whole batch in one call, filled in place (the argmax map is this function's own), histogram fused
            ops.fill_holes(pred, out=pred, truth=_to_u8_cuda(t, pred.device, 'truth'), ignore_index=ignore_value,
                           cm=self._cm())
            return
        ops.argmax_confusion(logits, truth, self.num_classes, out_size, ignore_index=ignore_value,
                             align_corners=align_corners, cm=self._cm())

    def sample_logits_tta(self, logits_list, flips, truth, out_size, ignore_value=255, align_corners=True):
        """sample_logits over the views of a batch (tta.TTA): the vote of ops.tta_vote in the place of the argmax."""
        if self.fill_holes:
            _, pred = ops.tta_vote(logits_list, flips, self.num_classes, out_size, align_corners=align_corners, want_pred=True)
            t = truth[:, 0] if truth.dim() == 4 else truth
            ops.fill_holes(pred, out=pred, truth=_to_u8_cuda(t, pred.device, 'truth'), ignore_index=ignore_value,
                           cm=self._cm())
            return
        ops.tta_vote(logits_list, flips, self.num_classes, out_size, labels=truth, ignore_index=ignore_value,
                     align_corners=align_corners, cm=self._cm())

    def sample_windows(self, logits_list, flips, view_sizes, windows, truth, out_size, ignore_value=255, align_corners=True):
        """sample_logits_tta over the window logits of a batch's views (tta.Windows): the stitch and vote of ops.window_vote in the
        place of the vote."""
        args = (logits_list, flips, view_sizes, windows.window, windows.stride, self.num_classes, out_size)
        if self.fill_holes:
            _, pred = ops.window_vote(*args, align_corners=align_corners, want_pred=True)
            t = truth[:, 0] if truth.dim() == 4 else truth
            ops.fill_holes(pred, out=pred, truth=_to_u8_cuda(t, pred.device, 'truth'), ignore_index=ignore_value,
                           cm=self._cm())
            return
        ops.window_vote(*args, labels=truth, ignore_index=ignore_value, align_corners=align_corners, cm=self._cm())

    def add_confusion(self, cm):
        """Add a batch's int64 (C,C) confusion matrix that is already on the device (EvaluatorCalibration.sample_views')."""
        self._cm().add_(cm)

    # reference attributes (float arrays, evaluation.py:49-51)
    @property
    def cm(self):
        return self._cm().cpu().numpy().astype(np.float64)

    @property
    def intersection(self):
        return np.diag(self.cm).copy()

    @property
    def union(self):
        cm = self.cm
        return cm.sum(axis=0) + cm.sum(axis=1) - np.diag(cm)

    def all_reduce(self, group=None):
        """Sum the confusion matrix over data-parallel ranks (validation set sharded by sample)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self._cm(), op=dist.ReduceOp.SUM, group=group)

    def score(self):
        return self.intersection.astype(float) / np.maximum(self.union.astype(float), 1.0)


# ------------------------------------------------------------------------------------------------------------------ calibration
CALIB_MAX_BINS, CALIB_MAX_TEMPS = 48, 8
CALIB_CONF_SCALE, CALIB_BRIER_SCALE, CALIB_NLL_SCALE = 2.0 ** 24, 2.0 ** 24, 2.0 ** 20
CALIB_DEFAULT_THRESHOLDS = (0.5, 0.9, 0.95, 0.97, 0.99)


def _numbers(text, what, example):
    parts = [p.strip() for p in str(text).split(',')]
    if not parts or any(p == '' for p in parts):
        raise ValueError('{} {!r}: expected a comma-separated list of numbers such as {}'.format(what, text, example))
    try:
        return tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError('{} {!r}: expected a comma-separated list of numbers such as {}'.format(what, text, example))


def parse_calibration_thresholds(text):
    """'0.5,0.9,0.97' -> (0.5, 0.9, 0.97); '' -> (). ValueError for anything that is not a list of numbers in (0, 1)."""
    if str(text).strip() == '':
        return ()
    return _checked_thresholds(_numbers(text, 'thresholds', '0.5,0.9,0.97'))


def parse_calibration_temperatures(text):
    """'0.5,2' -> (0.5, 2.0); '' -> (). ValueError for anything that is not a list of finite numbers > 0."""
    if str(text).strip() == '':
        return ()
    return _checked_temperatures(_numbers(text, 'temperatures', '0.5,0.75,1.5,2'))


def _checked_thresholds(thresholds):
    out = []
    for t in thresholds:
        t = float(t)
        if not 0.0 < t < 1.0 or not 0.0 < float(np.float32(t)) < 1.0:
            raise ValueError('thresholds: every threshold must lie inside (0, 1) as an fp32 number, got {!r}'.format(t))
        if float(np.float32(t)) in [float(np.float32(u)) for u in out]:
            raise ValueError('thresholds: {!r} is repeated'.format(t))
        out.append(t)
    return tuple(out)


def _checked_temperatures(temps):
    out = []
    for t in temps:
        t = float(t)
        with np.errstate(over='ignore'):
            t32 = float(np.float32(t))
        if not (t > 0.0) or math.isinf(t) or not (0.0 < t32 < float('inf')):
            raise ValueError('temperatures: every temperature must be a finite number > 0, got {!r}'.format(t))
        out.append(t)
    return tuple(out)


def calibration_edges(n_bins, thresholds):
    """The bin partition of a calibration report -> (edges, eq_bin, thr_bin): `edges` the fp32 interior edges, the sorted union of
    the equal-width edges i / n_bins and the thresholds (built in fp64, cast to fp32, duplicates merged) -- a confidence falls into
    bin #{j: edges[j] <= conf}; eq_bin[b] the equal-width bin that sub-bin b is a part of; thr_bin[i] the first sub-bin of the
    pixels with conf >= thresholds[i]. ValueError when n_bins is outside 1..48 or the union makes more than 48 bins."""
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= int(n_bins) <= CALIB_MAX_BINS:
        raise ValueError('bins: an integer in 1..{} is needed, got {!r}'.format(CALIB_MAX_BINS, n_bins))
    n_bins = int(n_bins)
    thresholds = _checked_thresholds(thresholds)
    eq = (np.arange(1, n_bins, dtype=np.float64) / n_bins).astype(np.float32)
    thr = np.asarray(thresholds, dtype=np.float64).astype(np.float32)
    edges = np.unique(np.concatenate([eq, thr]))
    if edges.size + 1 > CALIB_MAX_BINS:
        raise ValueError('{} bins and {} thresholds make {} bins; the kernel takes at most {}'.format(
            n_bins, len(thresholds), edges.size + 1, CALIB_MAX_BINS))
    lower = np.concatenate([np.zeros(1, dtype=np.float32), edges])           # the lower edge of every sub-bin
    eq_bin = np.searchsorted(eq, lower, side='right').astype(np.int64)       # #{i: eq_i <= lower}
    thr_bin = (np.searchsorted(edges, thr, side='left') + 1).astype(np.int64)
    return edges, eq_bin, thr_bin


class EvaluatorCalibration(object):
    """Calibration and pseudo-label quality of a model's confidence (this project's own definition; DESIGN 8, include/cutmixseg.h).
    `sample_views` is one launch of csrc/calib.hip per batch, which takes the place of the vote launch and ADDS exact integers into
    device-side tables: per (predicted class, confidence bin) the pixels, the correct pixels and the fixed-point confidence sum, plus
    the fixed-point Brier and NLL sums and a confusion matrix. They come to the host once, when a score is asked for, and every score
    is derived from them in fp64: the expected and maximum calibration error over `n_bins` equal-width bins (Naeini et al. 2015, Guo et
    al. 2017), NLL, Brier, the reliability table, and per threshold what a trainer's `--conf_thresh` would let through. `temperature`
    divides the logits before the softmax; `nll_temperatures` are up to seven more for the NLL alone."""

    def __init__(self, n_classes, n_bins=15, thresholds=CALIB_DEFAULT_THRESHOLDS, temperature=1.0, nll_temperatures=()):
        if not 1 <= int(n_classes) <= 64:
            raise ValueError('EvaluatorCalibration: 1 <= n_classes <= 64, got {}'.format(n_classes))
        self.num_classes = int(n_classes)
        self.edges, self.eq_bin, self.thr_bin = calibration_edges(n_bins, thresholds)
        self.n_bins = int(n_bins)
        self.thresholds = tuple(float(t) for t in thresholds)
        self.temperatures = _checked_temperatures((temperature,) + tuple(nll_temperatures))
        if len(self.temperatures) > CALIB_MAX_TEMPS:
            raise ValueError('temperatures: {} given, at most {} beside the histogram\'s'.format(
                len(self.temperatures) - 1, CALIB_MAX_TEMPS - 1))
        self.nb = int(self.edges.size) + 1
        self._dev = None
        self._host = None

    @property
    def temperature(self):
        return self.temperatures[0]

    # ---- the tables
    def _tables(self):
        if self._dev is None:
            dev, c = _device(), self.num_classes
            self._dev = (torch.zeros((c, self.nb, 3), dtype=torch.int64, device=dev),
                         torch.zeros((2 + len(self.temperatures),), dtype=torch.int64, device=dev),
                         torch.zeros((c, c), dtype=torch.int64, device=dev))
        return self._dev

    def sample_views(self, logits_list, flips, truth, out_size, ignore_value=255, align_corners=True, want_pred=False):
        """One batch: the views' low-resolution logits as ops.tta_vote takes them -> (the batch's own int64 (C,C) confusion matrix
        on the device, the uint8 prediction or None unless wanted), what ops.tta_vote returns."""
        hist, scores, own = self._tables()
        batch_cm, pred = ops.calibration_accumulate(logits_list, flips, self.num_classes, out_size, truth, self.edges,
                                                    np.asarray(self.temperatures, dtype=np.float32), hist, scores,
                                                    ignore_index=ignore_value, align_corners=align_corners, want_pred=want_pred)
        own += batch_cm                           # an integer add on the device: no host synchronisation
        self._host = None
        return batch_cm, pred

    def load_tables(self, hist, scores, cm):
        """Set the integer tables from host arrays (a saved `as_dict()`, a test): no GPU is needed for the derived scores."""
        c = self.num_classes
        hist, scores, cm = (np.asarray(a, dtype=np.int64) for a in (hist, scores, cm))
        if hist.shape != (c, self.nb, 3) or scores.shape != (2 + len(self.temperatures),) or cm.shape != (c, c):
            raise ValueError('load_tables: shapes {} / {} / {} expected'.format((c, self.nb, 3), (2 + len(self.temperatures),), (c, c)))
        self._host = (hist.copy(), scores.copy(), cm.copy())
        self._dev = None

    def tables(self):
        """-> (hist (C, nb, 3), scores (2 + nt,), cm (C, C)) int64 numpy"""
        if self._host is None:
            if self._dev is None:
                c = self.num_classes
                self._host = (np.zeros((c, self.nb, 3), dtype=np.int64), np.zeros(2 + len(self.temperatures), dtype=np.int64),
                              np.zeros((c, c), dtype=np.int64))
            else:
                self._host = tuple(t.cpu().numpy() for t in self._dev)
        return self._host

    # ---- derived scores, fp64 from the integers
    def _merged(self):
        """the sub-bins merged into the equal-width bins -> (n, correct, conf_sum), each (C, n_bins) float64"""
        hist = self.tables()[0]
        out = np.zeros((3, self.num_classes, self.n_bins))
        for b in range(self.nb):
            out[:, :, self.eq_bin[b]] += hist[:, b, :].T
        out[2] /= CALIB_CONF_SCALE
        return out

    @staticmethod
    def _gaps(n, correct, conf_sum):
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(n > 0, np.abs(correct / n - conf_sum / n), 0.0)

    def scored_pixels(self):
        return int(self.tables()[1][0])

    def ece(self):
        """sum over the equal-width bins of (n_b / N) |acc_b - conf_b|; NaN when no pixel was scored"""
        n, correct, conf = self._merged().sum(axis=1)
        total = n.sum()
        return float((n * self._gaps(n, correct, conf)).sum() / total) if total > 0 else float('nan')

    def ece_per_class(self):
        """-> (C,) the same over the pixels PREDICTED as each class; NaN for a class with none"""
        n, correct, conf = self._merged()
        total = n.sum(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(total > 0, (n * self._gaps(n, correct, conf)).sum(axis=1) / total, np.nan)

    def mce(self):
        n, correct, conf = self._merged().sum(axis=1)
        return float(self._gaps(n, correct, conf)[n > 0].max()) if (n > 0).any() else float('nan')

    def nll(self):
        """-> (nt,) the mean negative log-likelihood per temperature, temperatures[0] first"""
        scores = self.tables()[1]
        total = float(scores[0])
        return scores[2:].astype(np.float64) / CALIB_NLL_SCALE / total if total > 0 else np.full(len(self.temperatures), np.nan)

    def brier(self):
        scores = self.tables()[1]
        return float(scores[1]) / CALIB_BRIER_SCALE / float(scores[0]) if scores[0] > 0 else float('nan')

    def reliability(self):
        """-> [dict(lo, hi, n, acc, conf)] per equal-width bin; acc / conf NaN for an empty bin"""
        n, correct, conf = self._merged().sum(axis=1)
        rows = []
        for b in range(self.n_bins):
            nb_ = int(n[b])
            rows.append(dict(lo=b / self.n_bins, hi=(b + 1) / self.n_bins, n=nb_, acc=correct[b] / nb_ if nb_ else float('nan'),
                             conf=conf[b] / nb_ if nb_ else float('nan')))
        return rows

    def threshold_report(self):
        """-> per threshold dict(threshold, pass_rate, acc, acc_per_class (by predicted class), recall_per_class (by TRUE class:
        the share of its pixels that receive a correct pseudo-label)); NaN where there is no pixel"""
        hist, scores, cm = self.tables()
        total, truth = float(scores[0]), cm.sum(axis=1).astype(np.float64)
        out = []
        for t, s in zip(self.thresholds, self.thr_bin):
            n_c = hist[:, s:, 0].sum(axis=1).astype(np.float64)               # suffix sums over the bins at and above the threshold
            ok_c = hist[:, s:, 1].sum(axis=1).astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                out.append(dict(threshold=t, pass_rate=n_c.sum() / total if total > 0 else float('nan'),
                                acc=ok_c.sum() / n_c.sum() if n_c.sum() > 0 else float('nan'),
                                acc_per_class=np.where(n_c > 0, ok_c / n_c, np.nan),
                                recall_per_class=np.where(truth > 0, ok_c / truth, np.nan)))
        return out

    def as_dict(self):
        """Everything, JSON-serialisable: the settings, the integer tables and the derived scores (NaN as None)."""
        hist, scores, cm = self.tables()

        def clean(v):
            if isinstance(v, np.ndarray):
                return [clean(x) for x in v.tolist()]
            if isinstance(v, (list, tuple)):
                return [clean(x) for x in v]
            if isinstance(v, dict):
                return {k: clean(x) for k, x in v.items()}
            return None if isinstance(v, float) and v != v else v
        return clean(dict(n_classes=self.num_classes, n_bins=self.n_bins, thresholds=list(self.thresholds),
                          temperatures=list(self.temperatures), edges=[float(e) for e in self.edges], hist=hist, scores=scores, cm=cm,
                          scored_pixels=self.scored_pixels(), ece=self.ece(), ece_per_class=self.ece_per_class(), mce=self.mce(),
                          nll=self.nll(), brier=self.brier(), reliability=self.reliability(), thresholds_report=self.threshold_report()))
