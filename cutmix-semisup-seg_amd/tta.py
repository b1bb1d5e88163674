"""
Multi-scale / horizontal-flip test-time augmentation. The reference evaluates a network once per image, at the image's own size
(train_seg_semisup_mask_mt.py:510-514); DeepLab results on Pascal VOC and Cityscapes are usually reported as a vote over scaled and
mirrored views, which is what this adds on top of the reference.

A `TTA(scales, flip)` lists its views as (scale, flip) in the given scale order, each scale unflipped and then, with `flip`, flipped.
Per batch the padded evaluation canvas (DeviceAugmenter.stage_eval) is resampled once per view (ops.tta_resize; the view of the canvas'
own size is the canvas itself), every view goes through `net.forward_lowres`, and ONE launch of the vote kernel (ops.tta_vote,
csrc/tta.hip) turns the views' low-resolution logits into the uint8 prediction and the confusion matrix: the softmax probabilities
of the views, upsampled to the canvas and un-mirrored, summed in view order, argmax. Nothing of (N, C, H, W) is materialised. A single
view is scored on its logits, not its probabilities, so `TTA((1,), False)` is today's evaluation bit for bit.

torch is imported inside the functions: parsing `--scales` and refusing it loads no torch.
"""
import math

MAX_VIEWS = 16


def parse_scales(text):
    """'0.5,0.75,1' -> (0.5, 0.75, 1.0). ValueError for an empty or non-numeric list, a scale that is not a positive finite
    number, or a repeated scale."""
    parts = [p.strip() for p in str(text).split(',')]
    if not parts or any(p == '' for p in parts):
        raise ValueError('--scales {!r}: expected a comma-separated list of numbers such as 0.5,0.75,1'.format(text))
    try:
        scales = tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError('--scales {!r}: expected a comma-separated list of numbers such as 0.5,0.75,1'.format(text))
    return _checked_scales(scales)


def _checked_scales(scales):
    try:
        scales = tuple(float(s) for s in scales)
    except (TypeError, ValueError):
        raise ValueError('scales {!r}: expected numbers'.format(scales))
    if len(scales) == 0:
        raise ValueError('scales: at least one scale is needed')
    for s in scales:
        if not (s > 0.0) or math.isinf(s):
            raise ValueError('scales {!r}: every scale must be a positive finite number, got {}'.format(scales, s))
    if len(set(scales)) != len(scales):
        raise ValueError('scales {!r}: a scale is repeated'.format(scales))
    return scales


class TTA(object):
    def __init__(self, scales=(1.0,), flip=False):
        self.scales = _checked_scales(scales)
        self.flip = bool(flip)
        n_views = len(self.scales) * (2 if self.flip else 1)
        if n_views > MAX_VIEWS:
            raise ValueError('{} scales{} make {} views; the vote kernel takes at most {}'.format(
                len(self.scales), ' with --flip' if self.flip else '', n_views, MAX_VIEWS))

    def views(self):
        """[(scale, flip)] in the given scale order, each scale unflipped then flipped."""
        return [(s, f) for s in self.scales for f in ((False, True) if self.flip else (False,))]

    @staticmethod
    def _side(s, c, b):
        return b * max(1, int(math.floor(s * c / b + 0.5)))

    def view_size(self, canvas, block_size, scale=None):
        """The size of the view of `scale` (default: every scale, as a list) of a canvas: s * canvas rounded to the nearest multiple
        of the network's block size, at least one block."""
        (hc, wc), (bh, bw) = (int(v) for v in canvas), (int(v) for v in block_size)
        if scale is None:
            return [self.view_size(canvas, block_size, s) for s in self.scales]
        return self._side(scale, hc, bh), self._side(scale, wc, bw)

    def make_inputs(self, image, block_size):
        """image (N,C,Hc,Wc) CUDA -> [view tensor] in the order of views(). The unflipped view of the canvas' own size IS `image`."""
        from . import ops
        canvas = (int(image.shape[2]), int(image.shape[3]))
        out = []
        for s, f in self.views():
            size = self.view_size(canvas, block_size, s)
            out.append(image if (size == canvas and not f) else ops.tta_resize(image, size, flip=f))
        return out

    def predict(self, net, image, canvas, align_corners, labels=None, ignore_index=255, cm=None, want_pred=False,
                block_size=None, evaluator=None, calibration=None):
        """`net.forward_lowres` on every view of `image`, then one vote at `canvas` -> (cm | None, pred | None) as ops.tta_vote.
        With an `evaluator` (evaluation.EvaluatorIoU) the batch is counted into it (`sample_logits_tta`: its hole filling applies)
        instead of into `cm`, and the prediction, when wanted, is the plain vote, as the trainers save the plain argmax. With a
        `calibration` (evaluation.EvaluatorCalibration; labels are needed) its launch takes the place of the vote launch: it scores
        the confidence and gives the plain prediction and the confusion matrix that `evaluator` (or `cm`) then receives."""
        from . import ops
        logits = self.forward_views(net, image, block_size)
        flips = [f for _, f in self.views()]
        n_classes = int(logits[0].shape[1])
        if calibration is not None:
            fill = getattr(evaluator, 'fill_holes', False)
            batch_cm, pred = calibration.sample_views(logits, flips, labels, canvas, ignore_value=ignore_index,
                                                      align_corners=align_corners, want_pred=want_pred or fill)
            if evaluator is None:
                if cm is not None:
                    cm += batch_cm
                return (batch_cm if cm is None else cm), (pred if want_pred else None)
            if fill:
                evaluator.sample(labels[:, 0] if labels.dim() == 4 else labels, pred, ignore_value=ignore_index)
            else:
                evaluator.add_confusion(batch_cm)
            return None, (pred if want_pred else None)
        if evaluator is None:
            return ops.tta_vote(logits, flips, n_classes, canvas, labels=labels, ignore_index=ignore_index,
                                align_corners=align_corners, cm=cm, want_pred=want_pred)
        evaluator.sample_logits_tta(logits, flips, labels, canvas, ignore_value=ignore_index, align_corners=align_corners)
        if not want_pred:
            return None, None
        return ops.tta_vote(logits, flips, n_classes, canvas, align_corners=align_corners, want_pred=True)

    def forward_views(self, net, image, block_size=None):
        """-> the low-resolution logits of every view, in the order of views()"""
        if block_size is None:
            block_size = net.BLOCK_SIZE
        return [net.forward_lowres(x) for x in self.make_inputs(image, block_size)]

    def __repr__(self):
        return 'TTA(scales={}, flip={})'.format(self.scales, self.flip)
