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

With a `Windows(window, stride)` (eval_seg --window) every view is covered by overlapping windows of one size instead: one
ops.window_crop launch per view makes the window batch, the network sees the windows, and ONE launch of ops.window_vote
(csrc/window.hip) stitches and votes -- a pixel's score is the mean softmax probability of the windows that hold it, summed over the
views. include/cutmixseg.h states the grid; `Windows` carries the same arithmetic.

torch is imported inside the functions: parsing `--scales` / `--window` and refusing them loads no torch.
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


def parse_window(text, what='--window'):
    """'512,1024' -> (512, 1024), '513' -> (513, 513). ValueError for anything but one or two positive integers."""
    parts = [p.strip() for p in str(text).split(',')]
    try:
        if len(parts) not in (1, 2):
            raise ValueError
        vals = tuple(int(p) for p in parts)
    except ValueError:
        raise ValueError('{} {!r}: expected H,W or one integer, such as 512,1024 or 513'.format(what, text))
    if min(vals) < 1:
        raise ValueError('{} {!r}: every size must be at least 1'.format(what, text))
    return vals * 2 if len(vals) == 1 else vals


class Windows(object):
    """The sliding-window grid of include/cutmixseg.h: a window (wh, ww) and a stride (sh, sw), by default ceil(2 * window / 3) per
    axis, inside [ceil(window / 4), window]. Per view and axis: the effective window min(window, view); 1 window when it holds the
    view, else ceil((view - window) / stride) + 1; origins min(j * stride, view - effective window), the last window flush with the
    edge."""

    def __init__(self, window, stride=None):
        self.window = self._pair(window, 'window')
        self.stride = tuple(-(-2 * w // 3) for w in self.window) if stride is None else self._pair(stride, 'stride')
        for w, s in zip(self.window, self.stride):
            if s > w or s < -(-w // 4):
                raise ValueError('window stride {}x{}: each must lie in [ceil(window / 4), window] = [{}, {}] x [{}, {}]'.format(
                    self.stride[0], self.stride[1], -(-self.window[0] // 4), self.window[0], -(-self.window[1] // 4), self.window[1]))

    @staticmethod
    def _pair(v, what):
        try:
            v = (int(v),) * 2 if not hasattr(v, '__len__') else tuple(int(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError('{} {!r}: expected one integer or a pair'.format(what, v))
        if len(v) != 2 or min(v) < 1:
            raise ValueError('{} {!r}: expected one or two integers of at least 1'.format(what, v))
        return v

    def extent(self, view):
        """(eh, ew) of every window of a view of size `view`"""
        return tuple(min(w, int(v)) for w, v in zip(self.window, view))

    def grid(self, view):
        """(gy, gx)"""
        return tuple(1 if int(v) <= w else -(-(int(v) - w) // s) + 1 for v, w, s in zip(view, self.window, self.stride))

    def count(self, view):
        gy, gx = self.grid(view)
        return gy * gx

    def origins(self, view):
        """([y1_j], [x1_i])"""
        return tuple([min(j * s, int(v) - e) for j in range(g)]
                     for v, e, s, g in zip(view, self.extent(view), self.stride, self.grid(view)))

    def max_cover(self, view):
        """The largest number of windows that can hold one pixel of the view: per axis the ceil(extent / stride) regular windows a
        coordinate can lie in, one more when the flush last window is off the regular grid, never more than there are windows."""
        out = 1
        for v, e, s, g in zip(view, self.extent(view), self.stride, self.grid(view)):
            off_grid = g > 1 and (int(v) - e) % s != 0
            out *= min(g, -(-e // s) + (1 if off_grid else 0))
        return out

    def check_block(self, block_size):
        """ValueError unless the window is a multiple of the network's block size, naming the neighbouring multiples"""
        for axis, w, b in zip('HW', self.window, (int(v) for v in block_size)):
            if w % b:
                lo, hi = w // b * b, (w // b + 1) * b
                raise ValueError('window {}x{}: its {} of {} is not a multiple of the network\'s block size {}; the neighbouring '
                                 'multiples are {}'.format(self.window[0], self.window[1], 'height' if axis == 'H' else 'width', w, b,
                                                           '{} and {}'.format(lo, hi) if lo else str(hi)))

    def __repr__(self):
        return 'Windows(window={}, stride={})'.format(self.window, self.stride)


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
                block_size=None, evaluator=None, calibration=None, windows=None, window_batch=None):
        """`net.forward_lowres` on every view of `image`, then one vote at `canvas` -> (cm | None, pred | None) as ops.tta_vote.
        With `windows` (a Windows) every view is cut into its windows by one ops.window_crop launch, the windows go through the
        network in chunks of at most `window_batch` (default: the batch size), and one ops.window_vote launch stitches and votes;
        `evaluator` counts that batch through `sample_windows`, and `calibration` reads whole views, so it is refused beside it.
        With an `evaluator` (evaluation.EvaluatorIoU) the batch is counted into it (`sample_logits_tta`: its hole filling applies)
        instead of into `cm`, and the prediction, when wanted, is the plain vote, as the trainers save the plain argmax. With a
        `calibration` (evaluation.EvaluatorCalibration; labels are needed) its launch takes the place of the vote launch: it scores
        the confidence and gives the plain prediction and the confusion matrix that `evaluator` (or `cm`) then receives."""
        from . import ops
        if windows is not None:
            if calibration is not None:
                raise ValueError('predict: the calibration launch reads whole views, not windows')
            logits, sizes = self.forward_windows(net, image, windows, block_size, window_batch)
            flips = [f for _, f in self.views()]
            n_classes = int(logits[0].shape[1])
            args = (logits, flips, sizes, windows.window, windows.stride, n_classes, canvas)
            if evaluator is None:
                return ops.window_vote(*args, labels=labels, ignore_index=ignore_index, align_corners=align_corners, cm=cm,
                                       want_pred=want_pred)
            evaluator.sample_windows(logits, flips, sizes, windows, labels, canvas, ignore_value=ignore_index,
                                     align_corners=align_corners)
            if not want_pred:
                return None, None
            return ops.window_vote(*args, align_corners=align_corners, want_pred=True)
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

    def window_count(self, canvas, block_size, windows):
        """how many windows one image of a batch on `canvas` is forwarded as, over all views"""
        return sum(windows.count(self.view_size(canvas, block_size, s)) for s, _ in self.views())

    def forward_windows(self, net, image, windows, block_size=None, window_batch=None):
        """-> ([the window logits (N*G_i, C, hl, wl) of every view, one contiguous tensor each], [view sizes]) in the order of views().
        One ops.window_crop launch per view; the windows are forwarded in chunks of at most `window_batch` (default: N)."""
        import torch
        from . import ops
        if block_size is None:
            block_size = net.BLOCK_SIZE
        canvas = (int(image.shape[2]), int(image.shape[3]))
        chunk = int(image.shape[0]) if window_batch is None else int(window_batch)
        if chunk < 1:
            raise ValueError('window_batch must be at least 1, got {}'.format(window_batch))
        logits, sizes = [], []
        for s, f in self.views():
            size = self.view_size(canvas, block_size, s)
            crops = ops.window_crop(image, size, f, windows.window, windows.stride)
            total, out = int(crops.shape[0]), None
            for a in range(0, total, chunk):
                part = net.forward_lowres(crops[a:a + chunk])
                if out is None:
                    if int(part.shape[0]) == total:
                        out = part.contiguous()
                        break
                    out = torch.empty((total,) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
                out[a:a + int(part.shape[0])] = part
            logits.append(out)
            sizes.append(size)
        return logits, sizes

    def __repr__(self):
        return 'TTA(scales={}, flip={})'.format(self.scales, self.flip)
