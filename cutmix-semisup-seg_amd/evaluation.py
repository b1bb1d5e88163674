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
