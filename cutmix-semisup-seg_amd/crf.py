"""
CRF refinement of an evaluation batch's prediction against its image: a truncated, dilated-window form of the fully connected CRF
the DeepLab papers report their numbers after (include/cutmixseg.h and DESIGN 8 state the definition; the reference has nothing
of the kind). `CRFParams` holds the eight numbers (eval_seg's `--crf_*` options), checked against the kernel's limits; `refine_batch`
is the glue between DatasetRun.staged_eval and ops.crf_refine (csrc/crf.hip): the canvas' bytes, every image's rectangle on it, one
call per batch.

The defaults follow the DeepLab settings' weights (4 and 3) and colour bandwidth (13), with the window's reach (radius 5 x dilation
3 = 15 pixels) in the place of the dense kernel's theta_alpha. They are not tuned: no data set is at hand.

torch is imported inside the functions: parsing the options and refusing them loads no torch.
"""
import math

DEFAULTS = dict(iters=5, radius=5, dilation=3, bi_w=4.0, bi_xy=15.0, bi_rgb=13.0, pos_w=3.0, pos_xy=3.0)
LIMITS = dict(iters=(1, 32), radius=(1, 5), dilation=(1, 16))
WEIGHTS, THETAS = ('bi_w', 'pos_w'), ('bi_xy', 'bi_rgb', 'pos_xy')
FLOAT_MAX = 3.0e38


def _integer(name, value):
    if isinstance(value, bool):
        raise ValueError('crf {}: expected an integer, got {!r}'.format(name, value))
    try:
        v = int(str(value).strip()) if isinstance(value, str) else value
        if int(v) != v:
            raise ValueError
        v = int(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError('crf {}: expected an integer, got {!r}'.format(name, value))
    lo, hi = LIMITS[name]
    if not lo <= v <= hi:
        raise ValueError('crf {}: {} <= {} <= {}, got {}'.format(name, lo, name, hi, v))
    return v


def _number(name, value):
    if isinstance(value, bool):
        raise ValueError('crf {}: expected a number, got {!r}'.format(name, value))
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('crf {}: expected a number, got {!r}'.format(name, value))
    if not math.isfinite(v) or abs(v) > FLOAT_MAX:
        raise ValueError('crf {}: must be finite, got {}'.format(name, v))
    if name in WEIGHTS and v < 0.0:
        raise ValueError('crf {}: a weight is >= 0, got {}'.format(name, v))
    if name in THETAS and not v > 0.0:
        raise ValueError('crf {}: a bandwidth is > 0, got {}'.format(name, v))
    return v


class CRFParams(object):
    """iters, radius, dilation (integers inside the kernel's limits: 1..32, 1..5, 1..16), bi_w, bi_xy, bi_rgb (the appearance
    kernel's weight and its bandwidths in pixels and grey levels), pos_w, pos_xy (the smoothness kernel's). A value may be a number
    or its text; None takes the default. ValueError for anything else."""
    __slots__ = tuple(DEFAULTS)

    def __init__(self, **kw):
        unknown = sorted(set(kw) - set(DEFAULTS))
        if unknown:
            raise ValueError('crf: unknown parameter(s) {}'.format(', '.join(unknown)))
        for name, default in DEFAULTS.items():
            value = kw.get(name)
            value = default if value is None else value
            setattr(self, name, _integer(name, value) if name in LIMITS else _number(name, value))

    @classmethod
    def from_options(cls, enabled, **options):
        """eval_seg's options (crf_iters=..., None where not given) -> CRFParams, or None without `--crf`; a `--crf_*` value
        without `--crf` is a ValueError."""
        given = {k[len('crf_'):]: v for k, v in options.items() if v is not None}
        if not enabled:
            if given:
                raise ValueError('--crf_{} is given without --crf'.format(sorted(given)[0]))
            return None
        return cls(**given)

    def as_dict(self):
        return {k: getattr(self, k) for k in DEFAULTS}

    def __repr__(self):
        return 'CRFParams({})'.format(', '.join('{}={}'.format(k, getattr(self, k)) for k in DEFAULTS))


def rects_of(offsets, sizes):
    """stage_eval's `offsets` [(top, left)] and the pool's sizes [(h, w)] -> int32 (N,4) numpy (top, left, h, w)"""
    import numpy as np
    return np.array([[int(t), int(l), int(h), int(w)] for (t, l), (h, w) in zip(offsets, sizes)], dtype=np.int32).reshape(-1, 4)


def canvas_rgb(augment, pool, batch_ndx, block_size):
    """The evaluation canvas of stage_eval as bytes, (N,3,Hc,Wc) uint8 CUDA: the batch staged once more in fp32 by an augmenter of
    the same statistics and mapped back, round((x std + mean) 255) -- the pool's own bytes inside every rectangle (the staging
    kernel's (b / 255 - mean) / std is off by a few fp32 roundings, far below half a grey level); the padding is whatever 0 maps
    to and is never read as a neighbour."""
    import torch
    from .device_pipeline import DeviceAugmenter
    f32 = augment if augment.out_dtype == torch.float32 else DeviceAugmenter(augment.crop_size, augment.mean, augment.std,
                                                                             out_dtype=torch.float32)
    x = f32.stage_eval(pool, batch_ndx, block_size)['image']
    mean = torch.tensor([float(v) for v in augment.mean], dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor([float(v) for v in augment.std], dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    return ((x * std + mean) * 255.0).round_().clamp_(0.0, 255.0).to(torch.uint8)


def refine_batch(params, logits, flips, rgb, rects, n_classes, canvas, align_corners, stats_out=None):
    """-> (refined prediction uint8 (N,Hc,Wc), stats) of one evaluation batch (ops.crf_refine without labels: the caller counts)"""
    from . import ops
    _, pred, _, stats = ops.crf_refine(logits, flips, rgb, rects, n_classes, canvas, params, align_corners=align_corners,
                                       stats_out=stats_out)
    return pred, stats
