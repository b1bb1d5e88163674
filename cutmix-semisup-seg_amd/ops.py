"""
Tensor-level wrappers over the C ABI (include/cutmixseg.h). PyTorch is used for device memory, streams and
autograd plumbing only; all arithmetic happens in the HIP kernels. Every function requires CUDA(HIP) tensors and
raises otherwise -- there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import fn, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('cutmix-semisup-seg_amd ops run on the GPU only (got a {} tensor); there is no CPU '
                               'fallback'.format(t.device))


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _dtype_code(t):
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.bfloat16:
        return _lib.BF16
    raise TypeError('unsupported dtype {}'.format(t.dtype))


# ---------------------------------------------------------------------------------------------- box masks / paste
def ranges_to_device(ranges, device):
    """int32 (N, n_boxes, 4) numpy / tensor -> contiguous int32 CUDA tensor."""
    if isinstance(ranges, np.ndarray):
        ranges = torch.from_numpy(np.ascontiguousarray(ranges, dtype=np.int32))
    if not ranges.is_cuda and torch.device(device).type == 'cuda':
        # through PINNED memory: a "non_blocking" copy from pageable memory is a blocking one (the runtime stages it when the
        # stream gets there), i.e. the host would wait for the whole previous iteration at the first line of every iteration
        # and the GPU would then idle through the host's launch latencies (1 ms of a 19.9 ms step: profiles/r04k_*). The
        # caching host allocator keeps the staging block alive until the copy has run.
        ranges = ranges.to(torch.int32).contiguous().pin_memory()
    return ranges.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


def boxmask_rasterize(ranges, mask_shape, invert, out=None):
    """ranges int32 CUDA (N, nb, 4) -> f32 (N,1,H,W). mask_gen.py:110-116 on the device."""
    _need_cuda(ranges)
    n, nb = int(ranges.shape[0]), int(ranges.shape[1])
    H, W = int(mask_shape[0]), int(mask_shape[1])
    if out is None:
        out = torch.empty((n, 1, H, W), dtype=torch.float32, device=ranges.device)
    check(fn['cms_boxmask_rasterize'](_ptr(ranges), n, nb, H, W, int(bool(invert)), _ptr(out), _stream()),
          'cms_boxmask_rasterize')
    return out


def cutmix_paste(x0, x1, ranges=None, invert=True, mask=None, out=None):
    """
    out = x0*(1-m) + x1*m  (train_seg_semisup_mask_mt.py:350-351, 363); x0=None gives x1*m (:389).
    Give either int32 `ranges` (mask rasterised in-kernel) or a materialised f32 `mask` (N,1,H,W).
    """
    _need_cuda(x0, x1, ranges, mask)
    x1 = x1.contiguous()
    if x0 is not None:
        x0 = x0.contiguous()
        if x0.shape != x1.shape or x0.dtype != x1.dtype:
            raise ValueError('cutmix_paste: x0/x1 shape or dtype mismatch')
    n, c, h, w = (int(s) for s in x1.shape)
    if out is None:
        out = torch.empty_like(x1)
    dt = _dtype_code(x1)
    if (ranges is None) == (mask is None):
        raise ValueError('cutmix_paste: give exactly one of ranges / mask')
    if ranges is not None:
        check(fn['cms_cutmix_paste'](_ptr(x0), _ptr(x1), _ptr(out), dt, _ptr(ranges), n, int(ranges.shape[1]), c, h, w,
                                     int(bool(invert)), _stream()), 'cms_cutmix_paste')
    else:
        mask = _f32c(mask)
        check(fn['cms_cutmix_paste_mask'](_ptr(x0), _ptr(x1), _ptr(out), dt, _ptr(mask), n, c, h, w, _stream()),
              'cms_cutmix_paste_mask')
    return out


# ---------------------------------------------------------------------------------------------- consistency loss
def parse_class_thresh(text, n_classes=None):
    """--class_thresh: 'freematch', or comma-separated numbers in (0, 1] (one per class, checked once `n_classes` is known).
    -> 'freematch' or a list of floats; ValueError names what is wrong."""
    if isinstance(text, str) and text.strip().lower() == 'freematch':
        return 'freematch'
    if isinstance(text, str):
        try:
            vals = [float(v) for v in text.split(',')]
        except ValueError:
            raise ValueError("class_thresh must be 'freematch' or comma-separated numbers, got {!r}".format(text))
    else:
        vals = [float(v) for v in text]
    if len(vals) == 0 or not all(0.0 < v <= 1.0 for v in vals):      # (a NaN fails the comparison)
        raise ValueError('class_thresh: every threshold must be in (0, 1], got {}'.format(vals))
    if n_classes is not None and len(vals) != int(n_classes):
        raise ValueError('class_thresh lists {} thresholds for {} classes'.format(len(vals), int(n_classes)))
    return vals


class ClassThresholds(object):
    """Per-class confidence thresholds of the consistency loss and the device state behind them (csrc/cthresh.hip; definition in
    include/cutmixseg.h). mode='freematch': self-adaptive (FreeMatch without its fairness loss) -- tau, an EMA of the teacher's mean
    confidence, scaled per class by an EMA p~ of its mean class distribution, clamped to [floor, ceil]; both start at 1 / C. A list
    of C numbers: static thresholds. Every buffer is allocated once, so a captured graph replays against the same addresses:
        thr f32[C] | state f64[1 + C] = (tau, p~) | table u64[R][2 + 3C] of the iteration (R copies, summed) | epoch u64[1 + 2C].
    The consistency launches of an iteration add into `table`; `update()` (one launch, no host sync) folds the table of the
    PREVIOUS iteration ahead of the next one's launches; `pop_epoch_report()` is the one host synchronisation per epoch."""
    MAX_CLASSES = 128

    def __init__(self, n_classes, device, mode='freematch', ema=0.999, floor=0.0, ceil=0.97):
        C_ = int(n_classes)
        if not 1 <= C_ <= self.MAX_CLASSES:
            raise ValueError('ClassThresholds: 1..{} classes, got {}'.format(self.MAX_CLASSES, n_classes))
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('cutmix-semisup-seg_amd ops run on the GPU only (got device {}); there is no CPU fallback'.format(device))
        self.n_classes = C_
        self.adaptive = isinstance(mode, str)
        self.ema, self.floor, self.ceil = float(ema), float(floor), float(ceil)
        if not (0.0 <= self.ema < 1.0):
            raise ValueError('ClassThresholds: ema must be in [0, 1), got {}'.format(ema))
        if not (0.0 <= self.floor <= self.ceil <= 1.0 and self.ceil > 0.0):
            raise ValueError('ClassThresholds: need 0 <= floor <= ceil <= 1 and ceil > 0, got floor {} ceil {}'.format(floor, ceil))
        if self.adaptive:
            if parse_class_thresh(mode) != 'freematch':
                raise ValueError("ClassThresholds: mode must be 'freematch' or a list of thresholds")
            t0 = p0 = 1.0 / C_
            thr0 = np.full(C_, np.float32(min(self.ceil, max(self.floor, t0 * p0 / p0))), dtype=np.float32)
        else:
            thr0 = np.asarray(parse_class_thresh(mode, C_), dtype=np.float32)
        state0 = np.full(1 + C_, 1.0 / C_, dtype=np.float64)
        self.thr = torch.from_numpy(thr0).to(device)
        self.state = torch.from_numpy(state0).to(device)
        # (torch has no unsigned 64-bit arithmetic: int64 storage, the kernels see unsigned long long; counts stay far below 2^63)
        # (CTHRESH_REPLICAS copies: a workgroup adds into one of them, `iteration_table()` and the update launch sum them)
        self.table = torch.zeros((_lib.CTHRESH_REPLICAS, 2 + 3 * C_), dtype=torch.int64, device=device)
        self.epoch = torch.zeros(1 + 2 * C_, dtype=torch.int64, device=device)

    def iteration_table(self):
        """the iteration's table so far, int64[2 + 3C] on the device: the sum of the copies the launches add into"""
        return self.table.sum(dim=0)

    def update(self):
        """Fold the previous iteration's table (cms_cthresh_update) on the current stream. No host sync."""
        check(fn['cms_cthresh_update'](self.n_classes, int(self.adaptive), self.ema, self.floor, self.ceil, _ptr(self.state),
                                       _ptr(self.thr), _ptr(self.table), _ptr(self.epoch), _stream()), 'cms_cthresh_update')

    def pop_epoch_report(self):
        """The epoch's report, and the epoch counters cleared: dict(thr, tau, pixels, pass_rate) -- per class the valid pixels the
        teacher predicted as that class and the share of them that passed (None where there were none). ONE host synchronisation: the
        three buffers cross as one byte string. The counters are those `update()` has folded: a caller that wants the iteration just
        run in the report calls `update()` first (the trainer's hook does; the update at the head of the next step then finds an empty
        table and leaves everything as it is)."""
        C_ = self.n_classes
        raw = torch.cat([t.view(torch.uint8) for t in (self.state, self.epoch, self.thr)]).cpu().numpy()
        self.epoch.zero_()
        state = raw[:8 * (1 + C_)].view(np.float64)
        ep = raw[8 * (1 + C_):8 * (1 + C_) + 8 * (1 + 2 * C_)].view(np.uint64)
        thr = raw[8 * (2 + 3 * C_):].view(np.float32).copy()
        pred, passed = ep[1:1 + C_], ep[1 + C_:1 + 2 * C_]
        rate = [float(passed[c]) / float(pred[c]) if pred[c] > 0 else None for c in range(C_)]
        return dict(thr=thr, tau=float(state[0]), p=state[1:].copy(), n_valid=int(ep[0]), pixels=[int(v) for v in pred], pass_rate=rate)


class _LossConfig(object):
    """What the three consistency losses share: the per-pixel loss function, the confidence threshold and its mode, the upsample."""

    def __init__(self, loss_fn, conf_thresh, conf_per_pixel, align_corners, class_thresh=None):
        if loss_fn not in _lib.LOSS_IDS:
            raise ValueError('Unknown consistency loss function {}'.format(loss_fn))
        if class_thresh is not None and not isinstance(class_thresh, ClassThresholds):
            raise TypeError('class_thresh must be an ops.ClassThresholds or None')
        # per-class confidence thresholds (ClassThresholds) in the place of conf_thresh; None: the scalar threshold
        self.class_thresh = class_thresh
        self.loss_fn = loss_fn
        self.conf_thresh = float(conf_thresh)
        self.conf_per_pixel = bool(conf_per_pixel)
        self.align_corners = bool(align_corners)

    def fill(self, d):
        """the shared fields of a loss descriptor"""
        d.align_corners = int(self.align_corners)
        d.loss_fn = _lib.LOSS_IDS[self.loss_fn]
        d.conf_thresh = self.conf_thresh
        d.conf_per_pixel = int(self.conf_per_pixel)


class ConsistencyConfig(_LossConfig):
    """Static configuration of the unsupervised loss (train_seg_semisup_mask_mt.py CLI flags)."""

    def __init__(self, mode='mix', loss_fn='var', conf_thresh=0.97, conf_per_pixel=False, align_corners=True,
                 invert=True, class_thresh=None):
        if mode not in ('mix', 'cut'):
            raise ValueError('Unknown mask_mode {}'.format(mode))
        _LossConfig.__init__(self, loss_fn, conf_thresh, conf_per_pixel, align_corners, class_thresh)
        self.mode = mode
        self.invert = bool(invert)


def _nonempty_ranges(ranges):
    """(N, 0, 4) -- no box at all -- as ONE empty box per sample: a tensor without elements has no address, and the library would
    take the NULL pointer for "no ranges given". An empty box holds no pixel, so the parity of every pixel stays what zero boxes give."""
    if ranges is not None and ranges.dim() == 3 and ranges.shape[1] == 0:
        return torch.zeros((int(ranges.shape[0]), 1, 4), dtype=torch.int32, device=ranges.device)
    return ranges


def _cons_desc(cfg, l_stu, l_tea0, l_tea1, ranges, mask, um0, um1, out_size):
    n, c, h, w = (int(s) for s in l_stu.shape)
    d = _lib.ConsistencyDesc()
    d.l_stu, d.l_tea0, d.l_tea1 = l_stu.data_ptr(), l_tea0.data_ptr(), (l_tea1.data_ptr() if l_tea1 is not None else None)
    d.ranges = ranges.data_ptr() if ranges is not None else None
    d.mask = mask.data_ptr() if mask is not None else None
    d.um0 = um0.data_ptr() if um0 is not None else None
    d.um1 = um1.data_ptr() if um1 is not None else None
    d.n, d.c, d.h, d.w = n, c, h, w
    d.H, d.W = int(out_size[0]), int(out_size[1])
    cfg.fill(d)
    d.n_boxes = int(ranges.shape[1]) if ranges is not None else 0
    d.invert = int(cfg.invert)
    d.mode = _lib.MODE_MIX if cfg.mode == 'mix' else _lib.MODE_CUT
    return d


def _ct_desc(cfg, d):
    """the class-threshold descriptor around a consistency descriptor"""
    ct = cfg.class_thresh
    if int(d.c) != ct.n_classes:
        raise ValueError('consistency: logits have {} classes, the class thresholds {}'.format(int(d.c), ct.n_classes))
    cd = _lib.CthreshDesc()
    cd.cons = d
    cd.thr, cd.table = ct.thr.data_ptr(), ct.table.data_ptr()
    return cd


def _cons_family(cfg, d):
    """The entry point family `cfg` asks for and the descriptor it takes: cms_cthresh_* with the class-threshold descriptor around
    `d`, or cms_consistency_* with `d` itself."""
    if cfg.class_thresh is not None:
        return 'cms_cthresh_', _ct_desc(cfg, d)
    return 'cms_consistency_', d


def _cons_call(family, op, *args):
    """calls entry point `op` of a `_cons_family` on its descriptor and returns its value; an error code raises"""
    name = family[0] + op
    rc = fn[name](C.byref(family[1]), *args)
    if rc < 0:
        check(rc, name)
    return rc


def _workspace(name, d, device):
    """uninitialised scratch of the size cms_<name>_workspace_bytes asks for"""
    return _workspace_bytes(int(fn['cms_{}_workspace_bytes'.format(name)](C.byref(d))), device)


def _workspace_bytes(nbytes, device):
    """uninitialised scratch of `nbytes` (at least 16) from torch's caching allocator: no allocation call once the size has been seen"""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _check_grad_out(who, grad_out, like):
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != tuple(like.shape) or not grad_out.is_contiguous():
        raise ValueError('{}: grad_out must be a contiguous f32 tensor of the logits\' shape'.format(who))


def _finalized_scalars(stats, stats_g, cfg, ramp_val, cons_weight):
    """f32[4] [consistency_loss, conf_rate, grad_scale, unsup_loss] from the loss sums (`stats_g`: those of the global batch)"""
    scalars = torch.empty(4, dtype=torch.float32, device=stats.device)
    # (class thresholds are always on: the finalising launch only asks whether its threshold is positive)
    tau = 1.0 if getattr(cfg, 'class_thresh', None) is not None else cfg.conf_thresh
    check(fn['cms_consistency_finalize'](_ptr(stats), _ptr(stats_g), tau, int(cfg.conf_per_pixel),
                                         float(ramp_val), float(cons_weight), _ptr(scalars), _stream()),
          'cms_consistency_finalize')
    return scalars


def _allreduce_sum(t, group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return True
    return False


def _cons_prepare(who, cfg, l_stu, l_tea0, l_tea1, out_size, ranges, mask, um0, um1, grad_out=None):
    """The checks and conversions in front of a consistency launch: (descriptor, what the context keeps alive)."""
    _need_cuda(l_stu, l_tea0, l_tea1, ranges, mask, um0, um1, grad_out)
    l_stu, l_tea0, l_tea1 = _f32c(l_stu), _f32c(l_tea0), _f32c(l_tea1)
    mask, um0, um1 = _f32c(mask), _f32c(um0), _f32c(um1)
    ranges = _nonempty_ranges(ranges)
    if l_tea0.shape != l_stu.shape or (l_tea1 is not None and l_tea1.shape != l_stu.shape):
        raise ValueError('consistency: student / teacher logits shapes differ')
    if grad_out is not None:
        _check_grad_out(who, grad_out, l_stu)
    d = _cons_desc(cfg, l_stu, l_tea0, l_tea1, ranges, mask, um0, um1, out_size)
    return d, (l_stu, l_tea0, l_tea1, ranges, mask, um0, um1, cfg, tuple(int(v) for v in out_size))


def _cons_scalars(stats, cfg, ramp_val, cons_weight, group, sync_conf_rate):
    """the finalised scalars, with the confidence count of the global batch under torch.distributed"""
    stats_g = stats
    if sync_conf_rate and (cfg.conf_thresh > 0.0 or getattr(cfg, 'class_thresh', None) is not None):
        g = stats.clone()
        if _allreduce_sum(g, group):
            stats_g = g
    return _finalized_scalars(stats, stats_g, cfg, ramp_val, cons_weight)


def consistency_forward(cfg, l_stu, l_tea0, l_tea1, out_size, ranges=None, mask=None, um0=None, um1=None,
                        ramp_val=1.0, cons_weight=1.0, group=None, sync_conf_rate=True):
    """
    Fused forward. Returns (scalars, ctx): scalars = f32[4] device tensor
    [consistency_loss, conf_rate, grad_scale, unsup_loss]; ctx feeds consistency_backward. No host sync.
    Under torch.distributed the confidence count is all-reduced so that the rate is the global one.
    """
    d, keep = _cons_prepare('consistency_forward', cfg, l_stu, l_tea0, l_tea1, out_size, ranges, mask, um0, um1)
    dev = keep[0].device
    ws = _workspace('consistency', d, dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    _cons_call(_cons_family(cfg, d), 'fwd', _ptr(ws), _ptr(stats), _stream())
    return _cons_scalars(stats, cfg, ramp_val, cons_weight, group, sync_conf_rate), (d, keep, stats)


def consistency_backward(ctx, scalars, grad_out=None, samples=None):
    """grad wrt the (low-res) student logits; `grad_out` f32 (N,C,h,w) is accumulated into when given. `samples` = (s0, s1): only
    that run of samples (rows s0:s1 of `grad_out` are written) -- the per-pixel work of the backward is independent between samples,
    so a caller may issue disjoint runs on different streams (step.py: half of it on the main stream beside the other half)."""
    d, keep, _ = ctx
    l_stu, l_t0, l_t1, ranges, mask, um0, um1, cfg, out_size = keep
    if grad_out is None:
        grad_out = torch.zeros_like(l_stu)
    rows = grad_out
    if samples is not None:
        s0, s1 = int(samples[0]), int(samples[1])
        if not (0 <= s0 < s1 <= int(l_stu.shape[0])):
            raise ValueError('consistency_backward: bad sample range')
        sl = lambda t: None if t is None else t[s0:s1]
        d = _cons_desc(cfg, sl(l_stu), sl(l_t0), sl(l_t1), sl(ranges), sl(mask), sl(um0), sl(um1), out_size)
        rows = grad_out[s0:s1]
    _cons_call(_cons_family(cfg, d), 'bwd', _ptr(scalars), _ptr(rows), _stream())
    return grad_out


def consistency_fused(cfg, l_stu, l_tea0, l_tea1, out_size, grad_out, ranges=None, mask=None, um0=None, um1=None,
                      ramp_val=1.0, cons_weight=1.0, group=None, sync_conf_rate=True):
    """(round 6) `consistency_forward` + `consistency_backward` as ONE loss launch (cms_consistency_fwd_bwd): returns the same
    scalars and ADDS d unsup_loss / d l_stu to `grad_out` (f32 (N,C,h,w), its rows must be ZERO on entry: the deferred scalar factor
    -- the confidence rate of the default mode, in which the gradient is linear -- is applied to the rows afterwards). Falls back to
    the two launches where the fused one does not exist (identity geometry, deterministic mode, CMS_LOSS_FUSED=0)."""
    d, keep = _cons_prepare('consistency_fused', cfg, l_stu, l_tea0, l_tea1, out_size, ranges, mask, um0, um1, grad_out)
    l_stu, l_tea0, l_tea1, ranges, mask, um0, um1 = keep[:7]
    family = _cons_family(cfg, d)
    if not _cons_call(family, 'fused_supported'):
        sc, cctx = consistency_forward(cfg, l_stu, l_tea0, l_tea1, out_size, ranges, mask, um0, um1, ramp_val, cons_weight, group,
                                       sync_conf_rate)
        consistency_backward(cctx, sc, grad_out)
        return sc
    dev = l_stu.device
    ws = _workspace('consistency', d, dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    P = float(d.n) * float(d.H) * float(d.W)
    grad_unit = float(ramp_val) * float(cons_weight) / P
    _cons_call(family, 'fwd_bwd', grad_unit, _ptr(ws), _ptr(stats), _ptr(grad_out), _stream())
    scalars = _cons_scalars(stats, cfg, ramp_val, cons_weight, group, sync_conf_rate)
    if (cfg.class_thresh is not None or cfg.conf_thresh > 0.0) and not cfg.conf_per_pixel:
        # default confidence mode (:415-418): the loss mask is the scalar RATE -- the factor the launch above left out
        check(fn['cms_scale_by_scalar'](_ptr(grad_out), grad_out.numel(), _ptr(scalars), 1, 1.0, _stream()), 'cms_scale_by_scalar')
    return scalars


class _ConsistencyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l_stu, l_tea0, l_tea1, ranges, mask, um0, um1, cfg, out_size, ramp_val, cons_weight, group):
        scalars, c = consistency_forward(cfg, l_stu.detach(), l_tea0, l_tea1, out_size, ranges, mask, um0, um1,
                                         ramp_val, cons_weight, group)
        ctx.c = c
        ctx.scalars = scalars
        ctx.in_dtype = l_stu.dtype
        closs, rate, unsup = scalars[0], scalars[1], scalars[3]
        ctx.mark_non_differentiable(closs, rate)
        return unsup, closs, rate

    @staticmethod
    def backward(ctx, g_unsup, g_closs, g_rate):
        sc = ctx.scalars.clone()
        sc[2] = sc[2] * g_unsup
        grad = consistency_backward(ctx.c, sc)
        return (grad.to(ctx.in_dtype),) + (None,) * 11


def consistency_loss(l_stu, l_tea0, l_tea1, out_size, cfg, ranges=None, mask=None, um0=None, um1=None, ramp_val=1.0,
                     cons_weight=1.0, group=None):
    """autograd entry: returns (unsup_loss [differentiable wrt l_stu], consistency_loss, conf_rate)."""
    return _ConsistencyFn.apply(l_stu, l_tea0, l_tea1, ranges, mask, um0, um1, cfg, tuple(out_size), ramp_val,
                                cons_weight, group)


# ---------------------------------------------------------------------------------------------- ICT
def _lam_vector(lam, n):
    """mix factors as a contiguous f32 (N,) tensor: the reference keeps them as (N,1,1,1), train_seg_semisup_ict.py:306-307"""
    lam = _f32c(lam).reshape(-1)
    if int(lam.numel()) != int(n):
        raise ValueError('ict: {} mix factors for {} samples'.format(int(lam.numel()), int(n)))
    return lam


def ict_blend(x0, x1, lam, out=None):
    """out = x0*(1-lam) + x1*lam with one factor per sample (train_seg_semisup_ict.py:310-311): fp32 or bf16 (N, ...) tensors,
    arithmetic in fp32 with the reference's roundings. Images and validity masks."""
    _need_cuda(x0, x1, lam, out)
    if x0.shape != x1.shape or x0.dtype != x1.dtype:
        raise ValueError('ict_blend: x0/x1 shape or dtype mismatch')
    x0, x1 = x0.contiguous(), x1.contiguous()
    n = int(x0.shape[0])
    lam = _lam_vector(lam, n)
    if out is None:
        out = torch.empty_like(x0)
    elif out.shape != x0.shape or out.dtype != x0.dtype or not out.is_contiguous():
        raise ValueError('ict_blend: out must be a contiguous tensor of the inputs\' shape and dtype')
    if x0.numel() == 0:
        return out
    check(fn['cms_ict_blend'](_ptr(x0), _ptr(x1), _ptr(out), _dtype_code(x0), _ptr(lam), n, int(x0.numel()) // n, _stream()),
          'cms_ict_blend')
    return out


class ICTConsistencyConfig(_LossConfig):
    """Static configuration of the ICT loss (train_seg_semisup_ict.py CLI flags)."""

    def __init__(self, loss_fn='var', conf_thresh=0.97, conf_per_pixel=False, align_corners=True):
        _LossConfig.__init__(self, loss_fn, conf_thresh, conf_per_pixel, align_corners)


def ict_consistency_forward(cfg, l_stu, l_tea0, l_tea1, lam, out_size, um0=None, um1=None, ramp_val=1.0, cons_weight=1.0):
    """
    Fused ICT loss, forward (train_seg_semisup_ict.py:320-390). Returns (scalars, ctx) as consistency_forward does: scalars = f32[4]
    device tensor [consistency_loss, conf_rate, grad_scale, unsup_loss]; ctx feeds ict_consistency_backward. No host sync.
    """
    _need_cuda(l_stu, l_tea0, l_tea1, lam, um0, um1)
    l_stu, l_tea0, l_tea1 = _f32c(l_stu), _f32c(l_tea0), _f32c(l_tea1)
    um0, um1 = _f32c(um0), _f32c(um1)
    if l_tea0.shape != l_stu.shape or l_tea1.shape != l_stu.shape:
        raise ValueError('ict: student / teacher logits shapes differ')
    n, c, h, w = (int(s) for s in l_stu.shape)
    H, W = int(out_size[0]), int(out_size[1])
    for um in (um0, um1):
        if um is not None and int(um.numel()) != n * H * W:
            raise ValueError('ict: validity masks must be (N,1,H,W) of the loss geometry')
    lam = _lam_vector(lam, n)
    d = _lib.IctDesc()
    d.l_stu, d.l_tea0, d.l_tea1, d.lam = l_stu.data_ptr(), l_tea0.data_ptr(), l_tea1.data_ptr(), lam.data_ptr()
    d.um0 = um0.data_ptr() if um0 is not None else None
    d.um1 = um1.data_ptr() if um1 is not None else None
    d.n, d.c, d.h, d.w, d.H, d.W = n, c, h, w, H, W
    cfg.fill(d)
    dev = l_stu.device
    # the workspace goes into the context: the backward reads the confidence map of --conf_per_pixel from it
    ws = _workspace('ict', d, dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    check(fn['cms_ict_fwd'](C.byref(d), _ptr(ws), _ptr(stats), _stream()), 'cms_ict_fwd')
    keep = (l_stu, l_tea0, l_tea1, lam, um0, um1)
    return _finalized_scalars(stats, stats, cfg, ramp_val, cons_weight), (d, keep, ws, stats)


def ict_consistency_backward(ctx, scalars, grad_out=None):
    """fp32 gradient wrt the (low-res) student logits; `grad_out` f32 (N,C,h,w) is accumulated into when given."""
    d, keep, ws, _ = ctx
    if grad_out is None:
        grad_out = torch.zeros_like(keep[0])
    else:
        _check_grad_out('ict_consistency_backward', grad_out, keep[0])
    check(fn['cms_ict_bwd'](C.byref(d), _ptr(ws), _ptr(scalars), _ptr(grad_out), _stream()), 'cms_ict_bwd')
    return grad_out


# ---------------------------------------------------------------------------------------------- augmentation consistency
def aug_pixel_matrices(xf0_to_1, out_size, device=None):
    """
    The reference's `xf0_to_1` (N,2,3) -- the theta of F.affine_grid(..., align_corners=True), train_seg_semisup_aug_mt.py:302 --
    folded with the un-normalisation of F.grid_sample(align_corners=True) into pixel-space matrices: f32 (N,6) rows
    [a00 a01 a02 a10 a11 a12], a student pixel (x, y) samples the teacher's map at (a00 x + a01 y + a02, a10 x + a11 y + a12).
    The fold is done in float64 and rounded once. numpy / CPU tensors are folded on the host (and copied to `device` through
    pinned memory when one is given), device tensors on the device; no host synchronisation either way.
    """
    H, W = int(out_size[0]), int(out_size[1])
    if H < 2 or W < 2:
        raise ValueError('aug: the align_corners=True grid needs H >= 2 and W >= 2 (got {} x {})'.format(H, W))
    t = torch.as_tensor(xf0_to_1)
    if t.dim() != 3 or tuple(t.shape[1:]) != (2, 3):
        raise ValueError('aug: xf0_to_1 must be (N,2,3), got {}'.format(tuple(t.shape)))
    t = t.to(torch.float64)
    rx, ry = (W - 1) / 2.0, (H - 1) / 2.0
    a = torch.stack([t[:, 0, 0], t[:, 0, 1] * (rx / ry), (t[:, 0, 2] - t[:, 0, 0] - t[:, 0, 1] + 1.0) * rx,
                     t[:, 1, 0] * (ry / rx), t[:, 1, 1], (t[:, 1, 2] - t[:, 1, 0] - t[:, 1, 1] + 1.0) * ry], dim=1)
    a = a.to(torch.float32).contiguous()
    if device is not None and not a.is_cuda and torch.device(device).type == 'cuda':
        a = a.pin_memory().to(device, non_blocking=True)          # (pinned: see ranges_to_device)
    return a


class AugConsistencyConfig(_LossConfig):
    """Static configuration of the augmentation-consistency loss (train_seg_semisup_aug_mt.py CLI flags). `force_global`: never
    stage the teacher's rectangle in LDS (tests: both routes give the same bits)."""

    def __init__(self, loss_fn='var', conf_thresh=0.97, conf_per_pixel=False, align_corners=True, force_global=False):
        _LossConfig.__init__(self, loss_fn, conf_thresh, conf_per_pixel, align_corners)
        self.force_global = bool(force_global)


def aug_consistency_forward(cfg, l_stu, l_tea, xf0_to_1, out_size, um0=None, um1=None, ramp_val=1.0, cons_weight=1.0):
    """
    Fused affine-warp consistency loss, forward (train_seg_semisup_aug_mt.py:302-397): the teacher's prediction of view 0
    (`l_tea`, low-resolution logits) warped into the student's view 1 (`l_stu`) by `xf0_to_1` (N,2,3; numpy, CPU or device
    tensor). Returns (scalars, ctx) as consistency_forward does: scalars = f32[4] device tensor [consistency_loss, conf_rate,
    grad_scale, unsup_loss]; ctx feeds aug_consistency_backward. No host sync.
    """
    if not (torch.is_tensor(l_stu) and torch.is_tensor(l_tea) and l_stu.is_cuda and l_tea.is_cuda):
        raise ValueError('aug: the logits must be GPU tensors; there is no CPU fallback')
    _need_cuda(um0, um1)
    l_stu, l_tea = _f32c(l_stu), _f32c(l_tea)
    um0, um1 = _f32c(um0), _f32c(um1)
    if l_stu.dim() != 4 or l_tea.shape != l_stu.shape:
        raise ValueError('aug: student / teacher logits must be (N,C,h,w) of the same shape')
    n, c, h, w = (int(s) for s in l_stu.shape)
    H, W = int(out_size[0]), int(out_size[1])
    if h > H or w > W:
        raise ValueError('aug: logits larger than the loss geometry')
    for um in (um0, um1):
        if um is not None and (int(um.numel()) != n * H * W or int(um.shape[0]) != n):
            raise ValueError('aug: validity masks must be (N,1,H,W) of the loss geometry')
    xf = aug_pixel_matrices(xf0_to_1, (H, W), l_stu.device)
    if int(xf.shape[0]) != n:
        raise ValueError('aug: {} warp matrices for {} samples'.format(int(xf.shape[0]), n))
    d = _lib.AugDesc()
    d.l_stu, d.l_tea, d.xf = l_stu.data_ptr(), l_tea.data_ptr(), xf.data_ptr()
    d.um0 = um0.data_ptr() if um0 is not None else None
    d.um1 = um1.data_ptr() if um1 is not None else None
    d.n, d.c, d.h, d.w, d.H, d.W = n, c, h, w, H, W
    cfg.fill(d)
    d.force_global = int(cfg.force_global)
    dev = l_stu.device
    ws = _workspace('aug', d, dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    check(fn['cms_aug_fwd'](C.byref(d), _ptr(ws), _ptr(stats), _stream()), 'cms_aug_fwd')
    keep = (l_stu, l_tea, xf, um0, um1)
    return _finalized_scalars(stats, stats, cfg, ramp_val, cons_weight), (d, keep, ws, stats)


def aug_consistency_backward(ctx, scalars, grad_out=None):
    """fp32 gradient wrt the (low-res) student logits; `grad_out` f32 (N,C,h,w) is accumulated into when given."""
    d, keep, _, _ = ctx
    if grad_out is None:
        grad_out = torch.zeros_like(keep[0])
    else:
        _check_grad_out('aug_consistency_backward', grad_out, keep[0])
    check(fn['cms_aug_bwd'](C.byref(d), _ptr(scalars), _ptr(grad_out), _stream()), 'cms_aug_bwd')
    return grad_out


# ---------------------------------------------------------------------------------------------- supervised CE
def _ce_desc(logits, labels, ignore_index, out_size, align_corners):
    n, c, h, w = (int(s) for s in logits.shape)
    d = _lib.CeDesc()
    d.logits, d.labels = logits.data_ptr(), labels.data_ptr()
    if labels.dtype == torch.uint8:
        d.label_dtype = _lib.LABEL_U8
    elif labels.dtype == torch.int64:
        d.label_dtype = _lib.LABEL_I64
    else:
        raise TypeError('labels must be uint8 or int64, got {}'.format(labels.dtype))
    d.ignore_index = int(ignore_index)
    d.n, d.c, d.h, d.w = n, c, h, w
    d.H, d.W = int(out_size[0]), int(out_size[1])
    d.align_corners = int(bool(align_corners))
    return d


def _ce_prepare(logits, labels, out_size, ignore_index, align_corners, grad_out=None):
    """The checks and conversions in front of a cross-entropy launch: (descriptor, logits, labels)."""
    _need_cuda(logits, labels, grad_out)
    logits = _f32c(logits)
    labels = labels.contiguous()
    if labels.dim() == 4:
        labels = labels[:, 0].contiguous()
    if out_size is None:
        out_size = labels.shape[1:3]
    if tuple(labels.shape) != (logits.shape[0], int(out_size[0]), int(out_size[1])):
        raise ValueError('ce: labels shape {} does not match (N,H,W)=({}, {}, {})'.format(
            tuple(labels.shape), logits.shape[0], out_size[0], out_size[1]))
    if grad_out is not None:
        _check_grad_out('ce_fused', grad_out, logits)
    return _ce_desc(logits, labels, ignore_index, out_size, align_corners), logits, labels


def _ce_scalars(stats, loss_weight, group, sync_count):
    """(scalars f32[2] = [loss, grad_scale], the loss sums they were finalised from)"""
    if sync_count:
        # exact global-batch semantics under data parallelism: divide by the mean valid count over ranks
        import torch.distributed as dist
        cnt = stats[1:2].clone()
        if _allreduce_sum(cnt, group):
            stats = torch.stack([stats[0], cnt[0] / dist.get_world_size(group)])
    scalars = torch.empty(2, dtype=torch.float32, device=stats.device)
    check(fn['cms_ce_finalize'](_ptr(stats), float(loss_weight), _ptr(scalars), _stream()), 'cms_ce_finalize')
    return scalars, stats


def ce_forward(logits, labels, out_size=None, ignore_index=255, align_corners=True, loss_weight=1.0, group=None,
               sync_count=False):
    """labels (N,H,W) uint8/int64. Returns (scalars f32[2] = [loss, grad_scale], ctx)."""
    d, logits, labels = _ce_prepare(logits, labels, out_size, ignore_index, align_corners)
    ws = _workspace('ce', d, logits.device)
    stats = torch.empty(2, dtype=torch.float64, device=logits.device)
    check(fn['cms_ce_fwd'](C.byref(d), _ptr(ws), _ptr(stats), _stream()), 'cms_ce_fwd')
    scalars, stats = _ce_scalars(stats, loss_weight, group, sync_count)
    return scalars, (d, (logits, labels), stats)


def ce_fused(logits, labels, grad_out, out_size=None, ignore_index=255, align_corners=True, loss_weight=1.0, group=None,
             sync_count=False):
    """(round 6) `ce_forward` + `ce_backward` as ONE loss launch (cms_ce_fwd_bwd): returns the scalars f32[2] = [loss, grad_scale]
    and ADDS the gradient to `grad_out` (f32 (N,C,h,w), rows ZERO on entry: the factor loss_weight / count is applied afterwards)."""
    d, logits, labels = _ce_prepare(logits, labels, out_size, ignore_index, align_corners, grad_out)
    if not fn['cms_ce_fused_supported'](C.byref(d)):
        sc, cctx = ce_forward(logits, labels, out_size, ignore_index, align_corners, loss_weight, group, sync_count)
        ce_backward(cctx, sc, grad_out)
        return sc
    ws = _workspace('ce', d, logits.device)
    stats = torch.empty(2, dtype=torch.float64, device=logits.device)
    check(fn['cms_ce_fwd_bwd'](C.byref(d), _ptr(ws), _ptr(stats), _ptr(grad_out), _stream()), 'cms_ce_fwd_bwd')
    scalars, _ = _ce_scalars(stats, loss_weight, group, sync_count)
    check(fn['cms_scale_by_scalar'](_ptr(grad_out), grad_out.numel(), _ptr(scalars), 1, 1.0, _stream()), 'cms_scale_by_scalar')
    return scalars


def ce_backward(ctx, scalars, grad_out=None):
    d, keep, _ = ctx
    if grad_out is None:
        grad_out = torch.zeros_like(keep[0])
    check(fn['cms_ce_bwd'](C.byref(d), _ptr(scalars), _ptr(grad_out), _stream()), 'cms_ce_bwd')
    return grad_out


class _CeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, out_size, ignore_index, align_corners):
        scalars, c = ce_forward(logits.detach(), labels, out_size, ignore_index, align_corners)
        ctx.c = c
        ctx.scalars = scalars
        ctx.in_dtype = logits.dtype
        return scalars[0]

    @staticmethod
    def backward(ctx, g):
        sc = ctx.scalars.clone()
        sc[1] = sc[1] * g
        return ce_backward(ctx.c, sc).to(ctx.in_dtype), None, None, None, None


def cross_entropy(logits, labels, out_size=None, ignore_index=255, align_corners=True):
    """nn.CrossEntropyLoss(ignore_index)(upsample(logits), labels) with the upsample fused (pass full-res logits for
    the plain loss)."""
    return _CeFn.apply(logits, labels, None if out_size is None else tuple(out_size), ignore_index, align_corners)


# ---------------------------------------------------------------------------------------------- bilinear upsample
class _UpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, align_corners):
        _need_cuda(x)
        xin = _f32c(x)
        n, c, h, w = (int(s) for s in xin.shape)
        H, W = int(size[0]), int(size[1])
        out = torch.empty((n, c, H, W), dtype=torch.float32, device=x.device)
        check(fn['cms_upsample_bilinear_fwd'](_ptr(xin), _ptr(out), n, c, h, w, H, W, int(bool(align_corners)),
                                              _stream()), 'cms_upsample_bilinear_fwd')
        ctx.geo = (n, c, h, w, H, W, int(bool(align_corners)))
        ctx.in_dtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        n, c, h, w, H, W, ac = ctx.geo
        g = _f32c(g)
        gi = torch.empty((n, c, h, w), dtype=torch.float32, device=g.device)
        check(fn['cms_upsample_bilinear_bwd'](_ptr(g), _ptr(gi), n, c, h, w, H, W, ac, _stream()),
              'cms_upsample_bilinear_bwd')
        return gi.to(ctx.in_dtype), None, None


def upsample_bilinear(x, size, align_corners=True):
    return _UpsampleFn.apply(x, tuple(size), align_corners)


# ---------------------------------------------------------------------------------------------- stream pool
_STREAM_POOL = {}


_ROLE_ALIASES = {'optimizer': 'wgrad1'}      # roles that are never busy at the same time share one stream
_GOOD_STREAMS = {}          # device index -> candidate side streams that run CONCURRENTLY with the default stream (probed once)
_STREAM_PROBE_LOG = []


def _probe_side_streams(dev):
    """Side streams that really run beside the current stream AND beside each other. The runtime multiplexes streams onto a few
    hardware queues (4 here); which streams share one depends on what was created / used before (PyTorch's pool, RCCL, a
    notebook's leftovers), and two streams on one queue execute in order: a step whose teacher or weight-gradient stream shares
    a queue with the main stream -- or with each other -- loses 20-45 % (profiles/r05h_*, r05k_*, r05l_*: 482 img/s against 635 with
    ONE foreign stream created first). Probe (once per device and process, a few host synchronisations): every pair out of
    {current stream, six candidates} runs a ~100 us spin kernel side by side; same queue <=> the pair takes twice as long. Result:
    the largest set of candidates that overlap with the current stream and with one another (three, with four queues).
    CMS_STREAM_PROBE=0 switches the probe off (streams are then taken in creation order)."""
    good = _GOOD_STREAMS.get(dev.index)
    if good is not None:
        return good
    n_cand = 6
    cands = [torch.cuda.Stream(device=dev) for _ in range(n_cand)]
    if _os.environ.get('CMS_STREAM_PROBE', '1') == '0' or not hasattr(torch.cuda, '_sleep'):
        good = _GOOD_STREAMS[dev.index] = cands
        return good
    cur = torch.cuda.current_stream(dev)
    spin = 200000                                         # cycles of torch.cuda._sleep: ~0.1 ms
    streams = [cur] + cands

    def pair_ms(a, b):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(a)
        with torch.cuda.stream(a):
            torch.cuda._sleep(spin)
        if b is not None:
            b.wait_event(e0)
            with torch.cuda.stream(b):
                torch.cuda._sleep(spin)
            a.wait_stream(b)
        e1.record(a)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    with torch.cuda.device(dev):
        for st_ in streams:                               # every stream has run something: its queue is assigned
            with torch.cuda.stream(st_):
                torch.cuda._sleep(1000)
        n = len(streams)
        # The spin kernel counts SHADER clocks, so its duration moves with the power state (0.090 ms at 2.2 GHz, 0.150 ms right after
        # the GPU idled: tests/test_gpu_executor.py met that, round 6). A yardstick taken at a low clock would hide every clash
        # (2 x 0.09 < 1.5 x 0.15): a few ms of work bring the clock up first, the yardstick is measured before AND after the pairs,
        # and a probe whose two yardsticks disagree by more than 20 % is taken again (at most twice).
        for attempt in range(3):
            torch.cuda._sleep(20 * spin)
            pair_ms(cur, cands[0])                        # warm-up
            alone = max(min(pair_ms(cur, None) for _ in range(3)), 1e-3)
            clash = [[False] * n for _ in range(n)]

            def clashes(a, b):
                # noise (another process on the GPU, a second rank on the same device) only ever LENGTHENS a trial: a pair shares a
                # queue only if every one of three trials says so (one 0.1 ms timing per pair marked false clashes on a busy GPU)
                return all(pair_ms(a, b) >= 1.5 * alone for _ in range(3))
            for i in range(n):
                for j in range(i + 1, n):
                    clash[i][j] = clash[j][i] = clashes(streams[i], streams[j])
            alone_end = max(min(pair_ms(cur, None) for _ in range(3)), 1e-3)
            if 0.8 <= alone_end / alone <= 1.25:
                break
    # greedy: candidates in creation order that clash neither with the current stream nor with one already chosen
    chosen = []
    for j in range(1, n):
        if not clash[0][j] and all(not clash[j][k] for k in chosen):
            chosen.append(j)
    _STREAM_PROBE_LOG.append((dev.index, round(alone, 4), [[int(v) for v in row] for row in clash], [j - 1 for j in chosen]))
    good = [streams[j] for j in chosen]
    if len(good) < 3:
        # the step wants three side queues (teacher | two weight-gradient streams); say so instead of degrading silently
        import warnings
        warnings.warn('cutmix-semisup-seg_amd: the stream probe found {} side stream(s) that run beside the current stream and one '
                      'another (3 wanted){}; expect a slower step (roles share hardware queues). Clash matrix: {}'.format(
                          len(good), '' if len(good) >= 2 else ' -- falling back to creation order', _STREAM_PROBE_LOG[-1][2]),
                      RuntimeWarning, stacklevel=2)
    if len(good) < 2:                                     # a runtime this model does not fit: keep the creation order
        good = cands
    _GOOD_STREAMS[dev.index] = good
    return good


def probe_streams(device=None, again=False):
    """Run the side-stream probe NOW (instead of lazily inside the first step / recording) and return the clash log entry.
    `again=True` forgets the previous result AND the pooled role streams: call it after anything that creates streams of its own --
    `torch.distributed.init_process_group` + the first collective (RCCL's internal stream then exists and occupies a hardware queue,
    so the probe steers the step's roles away from it) -- and before the first step records its programs."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if again:
        _GOOD_STREAMS.pop(dev.index, None)
        for key in [k for k in _STREAM_POOL if k[0] == dev.index]:
            del _STREAM_POOL[key]
    _probe_side_streams(dev)
    return _STREAM_PROBE_LOG[-1] if _STREAM_PROBE_LOG else None


_SIDE_WORK = {}     # device index -> side streams holding weight-gradient launches the main stream has not joined yet
_SIDE_RR = {}       # device index -> round-robin counter over the two weight-gradient streams


_SIDE_SLOT = {}     # (device index, layer key) -> 0 / 1: a layer's weight gradients always go to the SAME side stream


_SIDE_ENABLED = True


def set_side_streams_enabled(on):
    """Switch the layer engines' side streams (weight gradients, ASPP branches) on / off; -> the previous setting. Off while a pass
    is captured into a hipGraph on ONE stream (graph_replay.GraphReplay.run)."""
    global _SIDE_ENABLED
    prev, _SIDE_ENABLED = _SIDE_ENABLED, bool(on)
    return prev


def side_streams_enabled():
    return _SIDE_ENABLED


def layer_wgrad_stream(device, key=None):
    """(round 6) Stream for ONE weight-gradient launch of the layer engines (backbone_hip._HipConvGeneralFn / _HipClassifierFn: the
    DeepLab v3+ head, the U-Nets), or None = issue it on the current stream. The autograd backward of those networks used to run
    data gradient -> weight gradient -> data gradient ... on ONE stream; the head of DeepLab v3+ alone is 10 ms of such a chain per
    66 ms step with a third of the CUs busy (profiles/r05b_step_timeline_v3plus.txt). Weight gradients feed nothing but the
    optimizer: they alternate over the two pooled weight-gradient streams, each forked from the current stream here (the operands
    are ready on it); `join_side_streams` is called by whatever touches the gradient arena next (optimizer launches, gradient
    clears, the bucketed all-reduce). Off under recording, in the deterministic mode (one shared split-K workspace) and with
    CMS_LAYER_WGRAD_SIDE=0."""
    if _REC is not None or _WGRAD_DETERMINISTIC or not _SIDE_ENABLED or _os.environ.get('CMS_LAYER_WGRAD_SIDE', '1') == '0':
        return None
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    # a LAYER keeps its stream (alternating in first-use order): a step with several backward passes (separate passes: cross
    # entropy, then consistency) adds to the same gradient twice, and the read-modify-write of a padded layer's scratch add is
    # ordered only within one stream
    slot = _SIDE_SLOT.get((idx, key))
    if slot is None:
        n = _SIDE_RR.get(idx, 0)
        _SIDE_RR[idx] = n + 1
        slot = _SIDE_SLOT[(idx, key)] = n & 1
    st = pooled_stream(dev, 'wgrad{}'.format(slot))
    cur = torch.cuda.current_stream(idx)
    if st.cuda_stream == cur.cuda_stream:
        return None
    st.wait_stream(cur)
    pend = _SIDE_WORK.setdefault(idx, [])
    if not pend:
        # first side launch of this backward pass: join when the pass ENDS (autograd runs the callback on the thread that called
        # .backward(), behind the last node), so that whoever reads or updates the gradients afterwards -- this package's fused
        # optimizers, a torch optimizer, a test -- sees them complete on its stream
        try:
            torch.autograd.Variable._execution_engine.queue_callback(lambda i=idx: join_side_streams(torch.device('cuda', i)))
        except RuntimeError:
            pass                         # (not inside a backward pass: the explicit joins -- optimizer, gradient clear -- remain)
    if all(p.cuda_stream != st.cuda_stream for p in pend):
        pend.append(st)
    return st


def join_side_streams(device=None):
    """The current stream waits for every weight-gradient launch `layer_wgrad_stream` put on a side stream since the last join."""
    if not _SIDE_WORK:
        return
    idx = None if device is None else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    pend = _SIDE_WORK.pop(idx, None)
    if pend:
        cur = torch.cuda.current_stream(idx)
        for st in pend:
            if st.cuda_stream != cur.cuda_stream:
                cur.wait_stream(st)


def pooled_stream(device, role):
    """A process-wide side stream per (device, role): roles 'teacher', 'wgrad0..2', 'side', 'optimizer'. HIP multiplexes its
    streams onto a handful of hardware queues; a process that keeps creating streams (bench.py runs four workloads, a
    notebook rebuilds its step object) ends up with its 'concurrent' streams on ONE queue and loses the overlap the step is
    built on (configs[1] without --freeze_bn as the fourth workload of one process: 277 img/s against 312 alone,
    profiles/r03also_*). Objects that need a side stream take it from here instead of creating their own.
    Round 5: (i) the streams come from a PROBED set that does not share the default stream's hardware queue (`_probe_side_streams`);
    (ii) roles that are never busy at the same time share one stream (`_ROLE_ALIASES`: the optimizer's early launch goes behind the
    second weight-gradient stream), so that the step needs fewer queues of its own."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    role = _ROLE_ALIASES.get(str(role), str(role))
    key = (dev.index, str(role))
    st = _STREAM_POOL.get(key)
    if st is None:
        # slot of a role among the probed streams: roles that run side by side sit on different slots -- teacher | first
        # weight-gradient stream (DeepLab v3+'s single one: 'side') | second weight-gradient stream (+ the optimizer's early launch)
        good = _probe_side_streams(dev)
        slot = {'teacher': 0, 'wgrad0': 1, 'side': 1, 'wgrad1': 2, 'wgrad2': 0}.get(role)
        if slot is None:
            slot = sum(1 for k in _STREAM_POOL if k[0] == dev.index)
        st = _STREAM_POOL[key] = good[slot % len(good)]
    return st


# ---------------------------------------------------------------------------------------------- NHWC data movement (v3+ head)
def _nhwc_ok(*ts):
    """contiguous NHWC bf16 / fp32 CUDA tensors with channels %% 8 == 0: what csrc/nhwc.hip takes."""
    for t in ts:
        if not (t.is_cuda and t.dim() == 4 and t.is_contiguous() and t.dtype in (torch.bfloat16, torch.float32)
                and t.shape[-1] % 8 == 0):
            return False
    return len({t.dtype for t in ts}) == 1


def _channel_copy(src, src_off, src_pitch, dst, dst_off, dst_pitch, rows, channels, row_div=1):
    es = src.element_size()
    check(fn['cms_channel_copy'](src.data_ptr() + src_off * es, int(src_pitch), dst.data_ptr() + dst_off * es, int(dst_pitch),
                                 int(rows), int(channels), _dtype_code(src), int(row_div), _stream()), 'cms_channel_copy')


class _ConcatChannelsFn(torch.autograd.Function):
    """torch.cat(dim = channels) of NHWC tensors; inputs of shape (N, 1, 1, C) are broadcast over the map (the pooled ASPP
    branch, deeplab3plus.py's F.interpolate of a 1 x 1 map). Backward: slice copies, pixel sums for the broadcast inputs."""

    @staticmethod
    def forward(ctx, *xs):
        # (every input 1 x 1 -- a feature map of one pixel: all of them share that geometry)
        big = next((x for x in xs if x.shape[1] * x.shape[2] > 1 or len(xs) == 1), xs[0])
        n, h, w = (int(v) for v in big.shape[:3])
        ctot = sum(int(x.shape[3]) for x in xs)
        out = torch.empty((n, h, w, ctot), dtype=big.dtype, device=big.device)
        off, meta = 0, []
        for x in xs:
            c = int(x.shape[3])
            bc = tuple(x.shape[1:3]) == (1, 1) and (h, w) != (1, 1)
            _channel_copy(x, 0, c, out, off, ctot, n * h * w, c, row_div=h * w if bc else 1)
            meta.append((off, c, bc))
            off += c
        ctx.meta, ctx.geo = meta, (n, h, w, ctot)
        return out

    @staticmethod
    def backward(ctx, g):
        n, h, w, ctot = ctx.geo
        g = g.contiguous()
        outs = []
        for i, (off, c, bc) in enumerate(ctx.meta):
            if not ctx.needs_input_grad[i]:
                outs.append(None)
            elif bc:
                acc = torch.empty((n, c), dtype=torch.float32, device=g.device)
                check(fn['cms_rows_reduce'](g.data_ptr() + off * g.element_size(), ctot, n, h * w, c, _dtype_code(g), _ptr(acc),
                                            1.0, _stream()), 'cms_rows_reduce')
                outs.append(acc.to(g.dtype).view(n, 1, 1, c))
            else:
                d = torch.empty((n, h, w, c), dtype=g.dtype, device=g.device)
                _channel_copy(g, off, ctot, d, 0, c, n * h * w, c)
                outs.append(d)
        return tuple(outs)


def concat_channels(xs):
    """NHWC tensors (N,H,W,Ci) [or (N,1,1,Ci): broadcast] -> (N,H,W,sum Ci) on csrc/nhwc.hip."""
    xs = [x if x.is_contiguous() else x.contiguous() for x in xs]
    if not _nhwc_ok(*xs):
        raise ValueError('concat_channels: contiguous NHWC bf16 / fp32 CUDA tensors with channels % 8 == 0 required')
    return _ConcatChannelsFn.apply(*xs)


class _UpsampleConcatFn(torch.autograd.Function):
    """cat([low, bilinear_upsample(x -> low's size)], channels) in one buffer (deeplab3plus.py:54-55 of the reference:
    F.interpolate(..., mode='bilinear', align_corners=False) then torch.cat) -- NHWC, the upsample written straight into its
    channel slice; backward = slice copy + the gather-form adjoint of the interpolation."""

    @staticmethod
    def forward(ctx, low, x, align_corners):
        n, H, W, cl = (int(v) for v in low.shape)
        _, h, w, cx = (int(v) for v in x.shape)
        out = torch.empty((n, H, W, cl + cx), dtype=low.dtype, device=low.device)
        _channel_copy(low, 0, cl, out, 0, cl + cx, n * H * W, cl)
        check(fn['cms_upsample_nhwc'](_ptr(x), out.data_ptr() + cl * out.element_size(), cl + cx, n, h, w, H, W, cx,
                                      _dtype_code(x), int(bool(align_corners)), 0, _stream()), 'cms_upsample_nhwc')
        ctx.geo = (n, H, W, cl, h, w, cx, bool(align_corners))
        return out

    @staticmethod
    def backward(ctx, g):
        n, H, W, cl, h, w, cx, align = ctx.geo
        g = g.contiguous()
        dlow = dx = None
        if ctx.needs_input_grad[0]:
            dlow = torch.empty((n, H, W, cl), dtype=g.dtype, device=g.device)
            _channel_copy(g, 0, cl + cx, dlow, 0, cl, n * H * W, cl)
        if ctx.needs_input_grad[1]:
            dx = torch.empty((n, h, w, cx), dtype=g.dtype, device=g.device)
            check(fn['cms_upsample_nhwc'](g.data_ptr() + cl * g.element_size(), _ptr(dx), cl + cx, n, h, w, H, W, cx,
                                          _dtype_code(g), int(align), 1, _stream()), 'cms_upsample_nhwc')
        return dlow, dx, None


def upsample_concat(low, x, align_corners=False):
    low = low if low.is_contiguous() else low.contiguous()
    x = x if x.is_contiguous() else x.contiguous()
    if not _nhwc_ok(low, x) or low.shape[0] != x.shape[0]:
        raise ValueError('upsample_concat: contiguous NHWC bf16 / fp32 CUDA tensors with channels % 8 == 0 required')
    return _UpsampleConcatFn.apply(low, x, align_corners)


class _GlobalAvgPoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d(1) on NHWC: (N,H,W,C) -> (N,1,1,C), fp32 accumulation."""

    @staticmethod
    def forward(ctx, x):
        n, h, w, c = (int(v) for v in x.shape)
        acc = torch.empty((n, c), dtype=torch.float32, device=x.device)
        check(fn['cms_rows_reduce'](_ptr(x), c, n, h * w, c, _dtype_code(x), _ptr(acc), 1.0 / float(h * w), _stream()),
              'cms_rows_reduce')
        ctx.geo = (n, h, w, c)
        return acc.to(x.dtype).view(n, 1, 1, c)

    @staticmethod
    def backward(ctx, g):
        n, h, w, c = ctx.geo
        row = (g.reshape(n, c).float() * (1.0 / float(h * w))).to(g.dtype).contiguous()
        dx = torch.empty((n, h, w, c), dtype=g.dtype, device=g.device)
        _channel_copy(row, 0, c, dx, 0, c, n * h * w, c, row_div=h * w)
        return dx


def global_avg_pool(x):
    x = x if x.is_contiguous() else x.contiguous()
    if not _nhwc_ok(x):
        raise ValueError('global_avg_pool: contiguous NHWC bf16 / fp32 CUDA tensor with channels % 8 == 0 required')
    return _GlobalAvgPoolFn.apply(x)


class _FanoutFn(torch.autograd.Function):
    """k aliases of one tensor whose gradients are summed by ONE launch (cms_add_n) instead of autograd's k - 1 pairwise adds
    (the ASPP input feeds five branches: four 346 MB bf16 adds per cfg 4 pass)."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return tuple(x.view(x.shape) for _ in range(k))

    @staticmethod
    def backward(ctx, *gs):
        live = [g if g.is_contiguous() else g.contiguous() for g in gs if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        g0 = live[0]
        if not (g0.is_cuda and g0.dtype in (torch.bfloat16, torch.float32) and g0.numel() % 8 == 0 and len(live) <= 6
                and all(g.dtype == g0.dtype and g.shape == g0.shape for g in live)):
            out = live[0]
            for g in live[1:]:
                out = out + g
            return out, None
        out = torch.empty_like(g0)
        ptrs = (C.c_void_p * len(live))(*[g.data_ptr() for g in live])
        check(fn['cms_add_n'](ptrs, len(live), _ptr(out), g0.numel(), _dtype_code(g0), _stream()), 'cms_add_n')
        return out, None


def fanout(x, k):
    return _FanoutFn.apply(x, int(k))


# ---------------------------------------------------------------------------------------------- EMA
def ema_flat(tgt, src, alpha, tgt_bf16=None):
    """tgt = tgt*alpha + src*(1-alpha) over flat fp32 CUDA buffers, reference rounding (optim_weight_ema.py:21-25)."""
    _need_cuda(tgt, src, tgt_bf16)
    if tgt.dtype != torch.float32 or src.dtype != torch.float32 or not tgt.is_contiguous() or not src.is_contiguous():
        raise TypeError('ema_flat: contiguous float32 buffers required')
    if tgt.numel() != src.numel():
        raise ValueError('ema_flat: size mismatch')
    one_minus_alpha = 1.0 - float(alpha)      # Python double, cast to fp32 at the ABI like the tensor-scalar mul
    check(fn['cms_ema_flat'](_ptr(tgt), _ptr(src), tgt.numel(), float(alpha), one_minus_alpha, _ptr(tgt_bf16),
                             _stream()), 'cms_ema_flat')
    return tgt


# ---------------------------------------------------------------------------------------------- evaluation
def argmax_confusion(logits, labels, num_classes, out_size=None, ignore_index=255, align_corners=True, cm=None,
                     want_pred=False):
    """
    Fused upsample + argmax + confusion matrix (train_seg_semisup_mask_mt.py:510-514, evaluation.py:6-37).
    labels (N,H,W) uint8/int64 or None. Returns (cm int64 (C,C) CUDA [accumulated into `cm` when given], pred|None).
    """
    _need_cuda(logits, labels, cm)
    logits = _f32c(logits)
    n, c, h, w = (int(s) for s in logits.shape)
    if c != num_classes:
        raise ValueError('argmax_confusion: logits have {} classes, expected {}'.format(c, num_classes))
    ldt = _lib.LABEL_U8
    if labels is not None:
        if labels.dim() == 4:
            labels = labels[:, 0]
        labels = labels.contiguous()
        ldt = _lib.LABEL_U8 if labels.dtype == torch.uint8 else _lib.LABEL_I64
        if labels.dtype not in (torch.uint8, torch.int64):
            raise TypeError('labels must be uint8 or int64')
        if out_size is None:
            out_size = labels.shape[1:3]
    if out_size is None:
        out_size = (h, w)
    H, W = int(out_size[0]), int(out_size[1])
    if labels is not None and cm is None:
        cm = torch.zeros((c, c), dtype=torch.int64, device=logits.device)
    pred = torch.empty((n, H, W), dtype=torch.uint8, device=logits.device) if want_pred else None
    check(fn['cms_argmax_confusion'](_ptr(logits), _ptr(labels), ldt, -1 if ignore_index is None else int(ignore_index),
                                     n, c, h, w, H, W, int(bool(align_corners)), _ptr(cm), _ptr(pred), _stream()),
          'cms_argmax_confusion')
    return cm, pred


def confusion(truth, pred, num_classes, ignore_index=None, cm=None):
    """uint8 CUDA maps of equal shape -> int64 (C,C) confusion matrix (row = truth, column = prediction)."""
    _need_cuda(truth, pred, cm)
    truth = truth.contiguous()
    pred = pred.contiguous()
    if truth.dtype != torch.uint8 or pred.dtype != torch.uint8:
        raise TypeError('confusion: uint8 maps required')
    if truth.numel() != pred.numel():
        raise ValueError('confusion: size mismatch')
    if cm is None:
        cm = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=truth.device)
    check(fn['cms_confusion'](_ptr(truth), _ptr(pred), truth.numel(), -1 if ignore_index is None else int(ignore_index),
                              int(num_classes), _ptr(cm), _stream()), 'cms_confusion')
    return cm


def fill_holes(pred, out=None, truth=None, ignore_index=None, cm=None):
    """
    scipy.ndimage.binary_fill_holes(pred != 0) on the device, bit-identical (evaluation.py:53-55). pred uint8 CUDA (H,W) or
    (N,H,W), each image filled on its own; `out` (same shape, {0,1}) may be `pred` itself. With `truth` (uint8, same shape)
    the 2 x 2 confusion matrix of (truth, filled) is accumulated into `cm` in the same launches. Returns (out, cm|None).
    """
    _need_cuda(pred, out, truth, cm)
    if pred.dtype != torch.uint8 or (truth is not None and truth.dtype != torch.uint8):
        raise TypeError('fill_holes: uint8 maps required')
    if pred.dim() not in (2, 3):
        raise ValueError('fill_holes: pred must be (H,W) or (N,H,W)')
    if cm is not None and truth is None:
        raise ValueError('fill_holes: cm given without truth')
    pred = pred.contiguous()
    if out is None:
        out = torch.empty_like(pred)
    elif out.dtype != torch.uint8 or not out.is_contiguous():
        raise TypeError('fill_holes: out must be a contiguous uint8 map')
    if out.shape != pred.shape or (truth is not None and truth.shape != pred.shape):
        raise ValueError('fill_holes: size mismatch')
    n = int(pred.shape[0]) if pred.dim() == 3 else 1
    h, w = int(pred.shape[-2]), int(pred.shape[-1])
    if truth is not None:
        truth = truth.contiguous()
        if cm is None:
            cm = torch.zeros((2, 2), dtype=torch.int64, device=pred.device)
        elif cm.dtype != torch.int64 or tuple(cm.shape) != (2, 2) or not cm.is_contiguous():
            raise TypeError('fill_holes: cm must be a contiguous int64 (2,2) matrix')
    nbytes = int(fn['cms_fill_holes_workspace_bytes'](n, h, w))
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=pred.device)
    check(fn['cms_fill_holes'](_ptr(pred), _ptr(out), _ptr(truth), -1 if ignore_index is None else int(ignore_index),
                               _ptr(cm), n, h, w, _ptr(ws), nbytes, _stream()), 'cms_fill_holes')
    return out, cm


# ---------------------------------------------------------------------------------------------- test-time augmentation
def _size2(size, what):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise TypeError('{} must be a pair of integers, got {!r}'.format(what, size))
    if h < 1 or w < 1:
        raise ValueError('{} must be at least 1 x 1, got {} x {}'.format(what, h, w))
    return h, w


def tta_resize(image, size, flip=False, out=None):
    """One view's input: image (N,C,H,W) fp32 / bf16 CUDA -> (N,C,Hs,Ws) of the same dtype, bilinear under align_corners=False
    without antialiasing, mirrored along x with `flip` (csrc/tta.hip). `out`: a contiguous tensor of that shape and dtype to fill."""
    if not torch.is_tensor(image) or image.dim() != 4:
        raise TypeError('tta_resize: image must be an (N,C,H,W) tensor')
    dtype = _dtype_code(image)
    hs, ws = _size2(size, 'tta_resize: size')
    _need_cuda(image, out)
    image = image.contiguous()
    n, c, h, w = (int(s) for s in image.shape)
    if min(n, c, h, w) < 1:
        raise ValueError('tta_resize: empty image {}'.format(tuple(image.shape)))
    if n * c * max(h * w, hs * ws) > 2 ** 31 - 1:
        raise ValueError('tta_resize: more than 2^31 - 1 elements')
    if out is None:
        out = torch.empty((n, c, hs, ws), dtype=image.dtype, device=image.device)
    elif out.dtype != image.dtype or not out.is_contiguous() or tuple(out.shape) != (n, c, hs, ws):
        raise TypeError('tta_resize: out must be a contiguous {} tensor of shape {}'.format(image.dtype, (n, c, hs, ws)))
    check(fn['cms_tta_resize'](_ptr(image), _ptr(out), n, c, h, w, hs, ws, dtype, int(bool(flip)), _stream()), 'cms_tta_resize')
    return out


def tta_vote(logits_list, flips, num_classes, out_size, labels=None, ignore_index=255, align_corners=True, cm=None,
             want_pred=False, pred=None):
    """
    The vote over the views of a batch (csrc/tta.hip): logits_list[i] (N,C,h_i,w_i) fp32 CUDA, flips[i] true where view i was
    computed on the mirrored input. One view: upsample + argmax, exactly argmax_confusion; more: the softmax probabilities of the
    views, each upsampled to `out_size` (a mirrored view read mirrored), summed in view order, argmax. labels (N,H,W) / (N,1,H,W)
    uint8 / int64 or None. `pred`: a contiguous uint8 (N,H,W) tensor to fill (implies want_pred). Returns (cm int64 (C,C) CUDA
    [accumulated into `cm` when given; None without labels], pred | None).
    """
    logits_list = list(logits_list)
    flips = [bool(f) for f in flips]
    k = len(logits_list)
    if k < 1 or k > _lib.TTA_MAX_VIEWS:
        raise ValueError('tta_vote: {} views, 1 to {} are built'.format(k, _lib.TTA_MAX_VIEWS))
    if len(flips) != k:
        raise ValueError('tta_vote: {} views but {} flips'.format(k, len(flips)))
    if any(not torch.is_tensor(t) or t.dim() != 4 for t in logits_list):
        raise TypeError('tta_vote: every view must be an (N,C,h,w) tensor')
    num_classes = int(num_classes)
    if num_classes < 1 or num_classes > 64:
        raise ValueError('tta_vote: 1 <= num_classes <= 64, got {}'.format(num_classes))
    H, W = _size2(out_size, 'tta_vote: out_size')
    n = int(logits_list[0].shape[0])
    for t in logits_list:
        if int(t.shape[0]) != n or int(t.shape[1]) != num_classes or min(int(s) for s in t.shape) < 1:
            raise ValueError('tta_vote: a view of shape {} among views of {} samples and {} classes'.format(
                tuple(t.shape), n, num_classes))
    if n * H * W > 2 ** 31 - 1:
        raise ValueError('tta_vote: more than 2^31 - 1 output pixels')
    if labels is not None:
        if not torch.is_tensor(labels) or labels.dtype not in (torch.uint8, torch.int64):
            raise TypeError('tta_vote: labels must be a uint8 or int64 tensor')
        if labels.dim() == 4:
            labels = labels[:, 0]
        if tuple(labels.shape) != (n, H, W):
            raise ValueError('tta_vote: labels of shape {}, {} expected'.format(tuple(labels.shape), (n, H, W)))
    if cm is not None:
        if labels is None:
            raise ValueError('tta_vote: cm given without labels')
        if cm.dtype != torch.int64 or tuple(cm.shape) != (num_classes, num_classes) or not cm.is_contiguous():
            raise TypeError('tta_vote: cm must be a contiguous int64 ({0},{0}) matrix'.format(num_classes))
    if pred is not None:
        if not torch.is_tensor(pred) or pred.dtype != torch.uint8 or not pred.is_contiguous() or tuple(pred.shape) != (n, H, W):
            raise TypeError('tta_vote: pred must be a contiguous uint8 tensor of shape {}'.format((n, H, W)))
        want_pred = True
    if labels is None and not want_pred:
        raise ValueError('tta_vote: nothing to produce (no labels and want_pred is False)')
    _need_cuda(labels, cm, pred, *logits_list)
    views = [_f32c(t) for t in logits_list]         # kept alive until the launch is queued
    dev = views[0].device
    if labels is not None:
        labels = labels.contiguous()
        if cm is None:
            cm = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=dev)
    if want_pred and pred is None:
        pred = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    d = _lib.TtaDesc()
    for i, t in enumerate(views):
        d.logits[i], d.h[i], d.w[i], d.flip[i] = t.data_ptr(), int(t.shape[2]), int(t.shape[3]), int(flips[i])
    d.n, d.c, d.H, d.W, d.k, d.align_corners = n, num_classes, H, W, k, int(bool(align_corners))
    d.labels = labels.data_ptr() if labels is not None else None
    d.label_dtype = _lib.LABEL_I64 if labels is not None and labels.dtype == torch.int64 else _lib.LABEL_U8
    d.ignore_index = -1 if ignore_index is None else int(ignore_index)
    d.cm = cm.data_ptr() if cm is not None else None
    d.pred_out = pred.data_ptr() if pred is not None else None
    check(fn['cms_tta_vote'](C.byref(d), _stream()), 'cms_tta_vote')
    return cm, pred


# ---------------------------------------------------------------------------------------------- sliding-window evaluation
def _window_grid(view, window, stride):
    """one axis of include/cutmixseg.h's window grid -> (windows, effective window)"""
    return (1 if view <= window else -(-(view - window) // stride) + 1), min(window, view)


def _window_pair(window, stride, what):
    (wh, ww), (sh, sw) = _size2(window, what + ': window'), _size2(stride, what + ': stride')
    for w, s in ((wh, sh), (ww, sw)):
        if s > w or s < -(-w // 4):
            raise ValueError('{}: stride {} x {} outside [ceil(window / 4), window] of the window {} x {}'.format(what, sh, sw, wh, ww))
    return wh, ww, sh, sw


def window_crop(image, view_size, flip, window, stride, out=None):
    """All windows of one view in one launch (csrc/window.hip): image (N,C,H,W) fp32 / bf16 CUDA -> (N*gy*gx, C, eh, ew) of the same
    dtype, window (j, i) of sample n being item (n*gy + j)*gx + i and bit for bit tta_resize(image, view_size, flip)[n, :, y1_j:y1_j+eh,
    x1_i:x1_i+ew]; the view is never materialised. `out`: a contiguous tensor of that shape and dtype to fill."""
    if not torch.is_tensor(image) or image.dim() != 4:
        raise TypeError('window_crop: image must be an (N,C,H,W) tensor')
    dtype = _dtype_code(image)
    hv, wv = _size2(view_size, 'window_crop: view_size')
    wh, ww, sh, sw = _window_pair(window, stride, 'window_crop')
    _need_cuda(image, out)
    image = image.contiguous()
    n, c, h, w = (int(s) for s in image.shape)
    if min(n, c, h, w) < 1:
        raise ValueError('window_crop: empty image {}'.format(tuple(image.shape)))
    (gy, eh), (gx, ew) = _window_grid(hv, wh, sh), _window_grid(wv, ww, sw)
    shape = (n * gy * gx, c, eh, ew)
    if max(n * c * h * w, shape[0] * c * eh * ew) > 2 ** 31 - 1:
        raise ValueError('window_crop: more than 2^31 - 1 elements')
    if out is None:
        out = torch.empty(shape, dtype=image.dtype, device=image.device)
    elif out.dtype != image.dtype or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError('window_crop: out must be a contiguous {} tensor of shape {}'.format(image.dtype, shape))
    check(fn['cms_window_crop'](_ptr(image), _ptr(out), n, c, h, w, hv, wv, int(bool(flip)), wh, ww, sh, sw, dtype, _stream()),
          'cms_window_crop')
    return out


def window_vote(logits, flips, view_sizes, window, stride, n_classes, size, labels=None, ignore_index=255, align_corners=True,
                cm=None, pred=None, want_pred=False):
    """
    The stitch and vote over the windows of the views of a batch (csrc/window.hip; include/cutmixseg.h states the definition):
    logits[i] (N*G_i, C, hl_i, wl_i) fp32 CUDA, the window batch of view i of size view_sizes[i], flips[i] true where the view was
    computed on the mirrored input; `window` / `stride` pairs of integers; `size` the canvas (H, W). A pixel's score is the sum over
    the views of the mean softmax probability of the windows that cover it; where no view has more than one window this is
    tta_vote, bit for bit. labels, cm, pred and the return value are tta_vote's.
    """
    logits = list(logits)
    flips = [bool(f) for f in flips]
    view_sizes = [_size2(v, 'window_vote: view size') for v in view_sizes]
    k = len(logits)
    if k < 1 or k > _lib.TTA_MAX_VIEWS:
        raise ValueError('window_vote: {} views, 1 to {} are built'.format(k, _lib.TTA_MAX_VIEWS))
    if len(flips) != k or len(view_sizes) != k:
        raise ValueError('window_vote: {} views but {} flips and {} view sizes'.format(k, len(flips), len(view_sizes)))
    if any(not torch.is_tensor(t) or t.dim() != 4 for t in logits):
        raise TypeError('window_vote: every view must be an (N*G,C,h,w) tensor')
    n_classes = int(n_classes)
    if n_classes < 1 or n_classes > 64:
        raise ValueError('window_vote: 1 <= n_classes <= 64, got {}'.format(n_classes))
    H, W = _size2(size, 'window_vote: size')
    wh, ww, sh, sw = _window_pair(window, stride, 'window_vote')
    grids = [(_window_grid(hv, wh, sh), _window_grid(wv, ww, sw)) for hv, wv in view_sizes]
    g0 = grids[0][0][0] * grids[0][1][0]
    if int(logits[0].shape[0]) % g0:
        raise ValueError('window_vote: {} window logits for a view of {} windows per sample'.format(int(logits[0].shape[0]), g0))
    n = int(logits[0].shape[0]) // g0
    for t, ((gy, eh), (gx, ew)) in zip(logits, grids):
        if int(t.shape[0]) != n * gy * gx or int(t.shape[1]) != n_classes or min(int(s) for s in t.shape) < 1:
            raise ValueError('window_vote: logits of shape {} for {} samples, {} x {} windows and {} classes'.format(
                tuple(t.shape), n, gy, gx, n_classes))
        if int(t.shape[2]) > eh or int(t.shape[3]) > ew:
            raise ValueError('window_vote: logits of {} x {} are larger than their window of {} x {}'.format(
                int(t.shape[2]), int(t.shape[3]), eh, ew))
        if t.numel() > 2 ** 31 - 1:
            raise ValueError('window_vote: more than 2^31 - 1 logits in a view')
    if n < 1:
        raise ValueError('window_vote: no samples')
    if n * H * W > 2 ** 31 - 1:
        raise ValueError('window_vote: more than 2^31 - 1 output pixels')
    if labels is not None:
        if not torch.is_tensor(labels) or labels.dtype not in (torch.uint8, torch.int64):
            raise TypeError('window_vote: labels must be a uint8 or int64 tensor')
        if labels.dim() == 4:
            labels = labels[:, 0]
        if tuple(labels.shape) != (n, H, W):
            raise ValueError('window_vote: labels of shape {}, {} expected'.format(tuple(labels.shape), (n, H, W)))
    if cm is not None:
        if labels is None:
            raise ValueError('window_vote: cm given without labels')
        if cm.dtype != torch.int64 or tuple(cm.shape) != (n_classes, n_classes) or not cm.is_contiguous():
            raise TypeError('window_vote: cm must be a contiguous int64 ({0},{0}) matrix'.format(n_classes))
    if pred is not None:
        if not torch.is_tensor(pred) or pred.dtype != torch.uint8 or not pred.is_contiguous() or tuple(pred.shape) != (n, H, W):
            raise TypeError('window_vote: pred must be a contiguous uint8 tensor of shape {}'.format((n, H, W)))
        want_pred = True
    if labels is None and not want_pred:
        raise ValueError('window_vote: nothing to produce (no labels and want_pred is False)')
    _need_cuda(labels, cm, pred, *logits)
    views = [_f32c(t) for t in logits]         # kept alive until the launch is queued
    dev = views[0].device
    if labels is not None:
        labels = labels.contiguous()
        if cm is None:
            cm = torch.zeros((n_classes, n_classes), dtype=torch.int64, device=dev)
    if want_pred and pred is None:
        pred = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    d = _lib.WindowDesc()
    for i, (t, ((gy, eh), (gx, ew))) in enumerate(zip(views, grids)):
        d.logits[i], d.hl[i], d.wl[i], d.flip[i] = t.data_ptr(), int(t.shape[2]), int(t.shape[3]), int(flips[i])
        d.Hv[i], d.Wv[i] = view_sizes[i]
        d.gy[i], d.gx[i], d.eh[i], d.ew[i], d.sh[i], d.sw[i] = gy, gx, eh, ew, sh, sw
    d.wh, d.ww = wh, ww
    d.n, d.c, d.H, d.W, d.k, d.align_corners = n, n_classes, H, W, k, int(bool(align_corners))
    d.labels = labels.data_ptr() if labels is not None else None
    d.label_dtype = _lib.LABEL_I64 if labels is not None and labels.dtype == torch.int64 else _lib.LABEL_U8
    d.ignore_index = -1 if ignore_index is None else int(ignore_index)
    d.cm = cm.data_ptr() if cm is not None else None
    d.pred_out = pred.data_ptr() if pred is not None else None
    check(fn['cms_window_vote'](C.byref(d), _stream()), 'cms_window_vote')
    return cm, pred


def calibration_accumulate(logits_list, flips, num_classes, out_size, labels, edges, temps, hist, scores, ignore_index=255,
                           align_corners=True, cm=None, want_pred=False, pred=None):
    """
    tta_vote with the confidence kept (csrc/calib.hip): one launch that ADDS, for every pixel with a valid label, into
      hist    int64 (C, nb, 3) CUDA, keyed by predicted class and confidence bin: pixels, correct pixels, sum of rint(conf * 2^24)
      scores  int64 (2 + nt,) CUDA: scored pixels, sum of rint(2^24 * squared error) at temps[0], per temperature sum of
              rint(2^20 * nll)
    `edges`: the nb - 1 strictly ascending interior bin edges in (0, 1) (a pixel is in bin #{j: edges[j] <= conf}, compared in fp32);
    `temps`: 1 to 8 temperatures, temps[0] the histogram's (and, with two or more views, the vote's). Views, labels, cm and pred as
    tta_vote's; labels are required. Returns (cm int64 (C,C) CUDA [accumulated into `cm` when given], pred | None). include/cutmixseg.h
    states the definition.
    """
    logits_list = list(logits_list)
    flips = [bool(f) for f in flips]
    k = len(logits_list)
    if k < 1 or k > _lib.TTA_MAX_VIEWS:
        raise ValueError('calibration_accumulate: {} views, 1 to {} are built'.format(k, _lib.TTA_MAX_VIEWS))
    if len(flips) != k:
        raise ValueError('calibration_accumulate: {} views but {} flips'.format(k, len(flips)))
    if any(not torch.is_tensor(t) or t.dim() != 4 for t in logits_list):
        raise TypeError('calibration_accumulate: every view must be an (N,C,h,w) tensor')
    num_classes = int(num_classes)
    if num_classes < 1 or num_classes > 64:
        raise ValueError('calibration_accumulate: 1 <= num_classes <= 64, got {}'.format(num_classes))
    H, W = _size2(out_size, 'calibration_accumulate: out_size')
    n = int(logits_list[0].shape[0])
    for t in logits_list:
        if int(t.shape[0]) != n or int(t.shape[1]) != num_classes or min(int(s) for s in t.shape) < 1:
            raise ValueError('calibration_accumulate: a view of shape {} among views of {} samples and {} classes'.format(
                tuple(t.shape), n, num_classes))
    if n * H * W > 2 ** 31 - 1:
        raise ValueError('calibration_accumulate: more than 2^31 - 1 output pixels')
    if not torch.is_tensor(labels) or labels.dtype not in (torch.uint8, torch.int64):
        raise TypeError('calibration_accumulate: labels must be a uint8 or int64 tensor')
    if labels.dim() == 4:
        labels = labels[:, 0]
    if tuple(labels.shape) != (n, H, W):
        raise ValueError('calibration_accumulate: labels of shape {}, {} expected'.format(tuple(labels.shape), (n, H, W)))
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float32).reshape(-1))
    temps = np.ascontiguousarray(np.asarray(temps, dtype=np.float32).reshape(-1))
    nb, nt = int(edges.size) + 1, int(temps.size)
    if nb > _lib.CALIB_MAX_BINS:
        raise ValueError('calibration_accumulate: {} bins, at most {} are built'.format(nb, _lib.CALIB_MAX_BINS))
    if nb > 1 and not (np.all(edges > 0) and np.all(edges < 1) and np.all(np.diff(edges) > 0)):
        raise ValueError('calibration_accumulate: edges must be strictly ascending inside (0, 1)')
    if nt < 1 or nt > _lib.CALIB_MAX_TEMPS:
        raise ValueError('calibration_accumulate: {} temperatures, 1 to {} are built'.format(nt, _lib.CALIB_MAX_TEMPS))
    if not (np.all(np.isfinite(temps)) and np.all(temps > 0)):
        raise ValueError('calibration_accumulate: every temperature must be finite and > 0, got {}'.format(temps.tolist()))
    for name, t, shape in (('hist', hist, (num_classes, nb, 3)), ('scores', scores, (2 + nt,))):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError('calibration_accumulate: {} must be a contiguous int64 tensor of shape {}'.format(name, shape))
    if cm is not None and (cm.dtype != torch.int64 or tuple(cm.shape) != (num_classes, num_classes) or not cm.is_contiguous()):
        raise TypeError('calibration_accumulate: cm must be a contiguous int64 ({0},{0}) matrix'.format(num_classes))
    if pred is not None:
        if not torch.is_tensor(pred) or pred.dtype != torch.uint8 or not pred.is_contiguous() or tuple(pred.shape) != (n, H, W):
            raise TypeError('calibration_accumulate: pred must be a contiguous uint8 tensor of shape {}'.format((n, H, W)))
        want_pred = True
    _need_cuda(labels, cm, pred, hist, scores, *logits_list)
    views = [_f32c(t) for t in logits_list]         # kept alive until the launch is queued
    dev = views[0].device
    labels = labels.contiguous()
    if cm is None:
        cm = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=dev)
    if want_pred and pred is None:
        pred = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    d = _lib.CalibDesc()
    for i, t in enumerate(views):
        d.logits[i], d.h[i], d.w[i], d.flip[i] = t.data_ptr(), int(t.shape[2]), int(t.shape[3]), int(flips[i])
    d.n, d.c, d.H, d.W, d.k, d.align_corners = n, num_classes, H, W, k, int(bool(align_corners))
    d.labels = labels.data_ptr()
    d.label_dtype = _lib.LABEL_I64 if labels.dtype == torch.int64 else _lib.LABEL_U8
    d.ignore_index = -1 if ignore_index is None else int(ignore_index)
    d.cm = cm.data_ptr()
    d.pred_out = pred.data_ptr() if pred is not None else None
    d.nb, d.edges = nb, (edges.ctypes.data if nb > 1 else None)      # host memory: read before the call returns
    d.nt, d.temps = nt, temps.ctypes.data
    d.hist, d.scores = hist.data_ptr(), scores.data_ptr()
    check(fn['cms_calib_accumulate'](C.byref(d), _stream()), 'cms_calib_accumulate')
    return cm, pred


CRF_LIMITS = dict(radius=(1, 5), dilation=(1, 16), iters=(1, 32))
CRF_WEIGHTS, CRF_THETAS = ('bi_w', 'pos_w'), ('bi_xy', 'bi_rgb', 'pos_xy')


def crf_checked_params(params):
    """`params` (crf.CRFParams, or anything with its eight attributes / keys) -> dict of plain numbers inside the kernel's limits;
    TypeError / ValueError otherwise. No torch, no GPU."""
    import math
    get = (lambda k: params[k]) if isinstance(params, dict) else (lambda k: getattr(params, k))
    out = {}
    try:
        for k, (lo, hi) in CRF_LIMITS.items():
            v = get(k)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError('crf_refine: {} must be an integer, got {!r}'.format(k, v))
            if not lo <= int(v) <= hi:
                raise ValueError('crf_refine: {} <= {} <= {}, got {}'.format(lo, k, hi, v))
            out[k] = int(v)
        for k in CRF_WEIGHTS + CRF_THETAS:
            v = float(get(k))
            if not math.isfinite(v) or v > 3.0e38 or (v < 0.0 if k in CRF_WEIGHTS else v <= 0.0):
                raise ValueError('crf_refine: {} must be finite and {} 0, got {}'.format(k, '>=' if k in CRF_WEIGHTS else '>', v))
            out[k] = v
    except (KeyError, AttributeError) as e:
        raise TypeError('crf_refine: params lacks {}'.format(e))
    return out


def _crf_rects(rects, n, H, W):
    """(n, 4) (top, left, h, w) on the HOST (numpy, list or CPU tensor) -> contiguous int32 numpy, every rectangle on the canvas"""
    if torch.is_tensor(rects):
        if rects.is_cuda:
            raise TypeError('crf_refine: rects must live on the host (they are checked before anything is launched)')
        rects = rects.numpy()
    r = np.asarray(rects)
    if r.dtype.kind not in 'iu' or r.shape != (n, 4):
        raise TypeError('crf_refine: rects must be an integer array of shape {}, got {} {}'.format((n, 4), r.dtype, r.shape))
    r = r.astype(np.int64)
    if (r[:, :2] < 0).any() or (r[:, 2:] < 1).any() or (r[:, 0] + r[:, 2] > H).any() or (r[:, 1] + r[:, 3] > W).any():
        raise ValueError('crf_refine: a rectangle is empty or leaves the {} x {} canvas: {}'.format(H, W, r.tolist()))
    return np.ascontiguousarray(r, dtype=np.int32)


def crf_refine(logits_list, flips, rgb, rects, num_classes, out_size, params, labels=None, ignore_index=255, align_corners=True,
               cm=None, pred=None, want_q=False, stats_out=None):
    """
    CRF refinement of the vote over the views of a batch against its image (csrc/crf.hip; include/cutmixseg.h states the
    definition): logits_list / flips as tta_vote's, rgb (N,3,H,W) uint8 CUDA, rects (N,4) = (top, left, h, w) of every image on the
    canvas, on the HOST, params a crf.CRFParams. labels (N,H,W) / (N,1,H,W) uint8 / int64 or None; `cm`, `pred`, `stats_out`
    (int64 [2]): contiguous CUDA tensors to accumulate into / fill. Returns (cm | None, pred uint8 (N,H,W), q fp32 (N,C,H,W) | None,
    stats int64 [2] = [pixels inside rectangles, of those the refined labels that differ from the unary ones]). Everything is
    refused before the GPU is touched; no host synchronisation.
    """
    prm = crf_checked_params(params)
    logits_list = list(logits_list)
    flips = [bool(f) for f in flips]
    k = len(logits_list)
    if k < 1 or k > _lib.TTA_MAX_VIEWS:
        raise ValueError('crf_refine: {} views, 1 to {} are built'.format(k, _lib.TTA_MAX_VIEWS))
    if len(flips) != k:
        raise ValueError('crf_refine: {} views but {} flips'.format(k, len(flips)))
    if any(not torch.is_tensor(t) or t.dim() != 4 for t in logits_list):
        raise TypeError('crf_refine: every view must be an (N,C,h,w) tensor')
    if any(t.dtype != torch.float32 for t in logits_list):
        raise TypeError('crf_refine: the views must be float32')
    num_classes = int(num_classes)
    if num_classes < 1 or num_classes > 64:
        raise ValueError('crf_refine: 1 <= num_classes <= 64, got {}'.format(num_classes))
    H, W = _size2(out_size, 'crf_refine: out_size')
    n = int(logits_list[0].shape[0])
    for t in logits_list:
        if int(t.shape[0]) != n or int(t.shape[1]) != num_classes or min(int(s) for s in t.shape) < 1:
            raise ValueError('crf_refine: a view of shape {} among views of {} samples and {} classes'.format(
                tuple(t.shape), n, num_classes))
    if n * H * W > 2 ** 31 - 1:
        raise ValueError('crf_refine: more than 2^31 - 1 output pixels')
    if not torch.is_tensor(rgb) or rgb.dtype != torch.uint8:
        raise TypeError('crf_refine: rgb must be a uint8 tensor')
    if tuple(rgb.shape) != (n, 3, H, W):
        raise ValueError('crf_refine: rgb of shape {}, {} expected'.format(tuple(rgb.shape), (n, 3, H, W)))
    rects = _crf_rects(rects, n, H, W)
    if labels is not None:
        if not torch.is_tensor(labels) or labels.dtype not in (torch.uint8, torch.int64):
            raise TypeError('crf_refine: labels must be a uint8 or int64 tensor')
        if labels.dim() == 4:
            labels = labels[:, 0]
        if tuple(labels.shape) != (n, H, W):
            raise ValueError('crf_refine: labels of shape {}, {} expected'.format(tuple(labels.shape), (n, H, W)))
    if cm is not None:
        if labels is None:
            raise ValueError('crf_refine: cm given without labels')
        if not torch.is_tensor(cm) or cm.dtype != torch.int64 or tuple(cm.shape) != (num_classes, num_classes) or not cm.is_contiguous():
            raise TypeError('crf_refine: cm must be a contiguous int64 ({0},{0}) matrix'.format(num_classes))
    if pred is not None:
        if not torch.is_tensor(pred) or pred.dtype != torch.uint8 or not pred.is_contiguous() or tuple(pred.shape) != (n, H, W):
            raise TypeError('crf_refine: pred must be a contiguous uint8 tensor of shape {}'.format((n, H, W)))
    if stats_out is not None:
        if (not torch.is_tensor(stats_out) or stats_out.dtype != torch.int64 or not stats_out.is_contiguous()
                or tuple(stats_out.shape) != (2,)):
            raise TypeError('crf_refine: stats_out must be a contiguous int64 tensor of 2 elements')
    _need_cuda(rgb, labels, cm, pred, stats_out, *logits_list)
    views = [t.contiguous() for t in logits_list]          # kept alive until the launches are queued
    dev = views[0].device
    rgb = rgb.contiguous()
    if labels is not None:
        labels = labels.contiguous()
        if cm is None:
            cm = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=dev)
    if pred is None:
        pred = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    q = torch.empty((n, num_classes, H, W), dtype=torch.float32, device=dev) if want_q else None
    stats = stats_out if stats_out is not None else torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = int(fn['cms_crf_workspace_bytes'](n, num_classes, H, W))
    work = _workspace_bytes(nbytes, dev)
    d = _lib.CrfDesc()
    for i, t in enumerate(views):
        d.logits[i], d.h[i], d.w[i], d.flip[i] = t.data_ptr(), int(t.shape[2]), int(t.shape[3]), int(flips[i])
    d.n, d.c, d.H, d.W, d.k, d.align_corners = n, num_classes, H, W, k, int(bool(align_corners))
    d.rgb, d.rect = rgb.data_ptr(), rects.ctypes.data
    d.radius, d.dilation, d.iters = prm['radius'], prm['dilation'], prm['iters']
    d.bi_w, d.bi_xy, d.bi_rgb, d.pos_w, d.pos_xy = prm['bi_w'], prm['bi_xy'], prm['bi_rgb'], prm['pos_w'], prm['pos_xy']
    d.labels = labels.data_ptr() if labels is not None else None
    d.label_dtype = _lib.LABEL_I64 if labels is not None and labels.dtype == torch.int64 else _lib.LABEL_U8
    d.ignore_index = -1 if ignore_index is None else int(ignore_index)
    d.cm = cm.data_ptr() if cm is not None else None
    d.pred_out, d.q_out, d.stats = pred.data_ptr(), (q.data_ptr() if q is not None else None), stats.data_ptr()
    check(fn['cms_crf_refine'](C.byref(d), _ptr(work), nbytes, _stream()), 'cms_crf_refine')
    return cm, pred, q, stats


# ---------------------------------------------------------------------------------------------- converter downsampling
def _downsample_u8(name, src, d, out, channels):
    _need_cuda(src, out)
    dims = 4 if channels == 3 else 3
    if src.dtype != torch.uint8 or src.dim() != dims or (channels == 3 and int(src.shape[-1]) != 3):
        raise TypeError('{}: a uint8 {} tensor is expected'.format(name, '(N,H,W,3)' if channels == 3 else '(N,H,W)'))
    src = src.contiguous()
    n, h, w, d = int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), int(d)
    if d < 1 or h % d or w % d:
        raise ValueError('{}: {}x{} is not divisible by d={}'.format(name, h, w, d))
    shape = (n, h // d, w // d) + ((3,) if channels == 3 else ())
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError('{}: out must be a contiguous uint8 tensor of shape {}'.format(name, shape))
    check(fn[name](_ptr(src), n, h, w, d, _ptr(out), _stream()), name)
    return out


def downsample_image_u8(src, d, out=None):
    """uint8 CUDA (N,H,W,3) -> (N,H/d,W/d,3): the mean of each d x d block per channel, truncated (the converter's
    downscale_local_mean(...).astype(uint8), exactly floor(sum / d^2)). d in 1..8 divides H and W."""
    return _downsample_u8('cms_downsample_image_u8', src, d, out, 3)


def downsample_labels_u8(src, d, out=None):
    """uint8 CUDA (N,H,W) -> (N,H/d,W/d): the most frequent value of each d x d block, the lowest value winning ties (the
    converter's one-hot sum and argmax)."""
    return _downsample_u8('cms_downsample_labels_u8', src, d, out, 1)


# ---------------------------------------------------------------------------------------------- converter area resize
def _u8_image_batch(name, src):
    """-> (contiguous src, channels) of a uint8 (N,H,W,3) or (N,H,W) tensor"""
    if src.dtype != torch.uint8 or src.dim() not in (3, 4) or (src.dim() == 4 and int(src.shape[-1]) != 3):
        raise TypeError('{}: a uint8 (N,H,W,3) or (N,H,W) tensor is expected'.format(name))
    return src.contiguous(), 3 if src.dim() == 4 else 1


def resize_area_u8(src, ho, wo, out=None):
    """uint8 CUDA (N,H,W,3) or (N,H,W) -> (N,ho,wo,3) or (N,ho,wo), ho <= H and wo <= W: the exact area filter of
    csrc/resize_math.hpp, sum wy wx p / (H W) rounded to nearest with ties to even. ho == H and wo == W copies."""
    name = 'cms_resize_area_u8'
    _need_cuda(src, out)
    src, c = _u8_image_batch(name, src)
    n, h, w, ho, wo = int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), int(ho), int(wo)
    if ho < 1 or wo < 1 or ho > h or wo > w:
        raise ValueError('{}: {}x{} -> {}x{}: the target must be at least 1x1 and no larger than the source'.format(name, h, w, ho, wo))
    shape = (n, ho, wo) + ((3,) if c == 3 else ())
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError('{}: out must be a contiguous uint8 tensor of shape {}'.format(name, shape))
    check(fn[name](_ptr(src), n, h, w, c, ho, wo, _ptr(out), _stream()), name)
    return out


def sum_sumsq_u8(src):
    """uint8 CUDA (N,H,W,3) or (N,H,W) -> int64 (N, 2C): per image the sum of the pixel values of each channel, then the sum of
    their squares (the converter's rgb_mean_std.pkl is made from these)."""
    name = 'cms_sum_sumsq_u8'
    _need_cuda(src)
    src, c = _u8_image_batch(name, src)
    n, pixels = int(src.shape[0]), int(src.shape[1]) * int(src.shape[2])
    if n < 1 or pixels < 1:
        raise ValueError('{}: an empty tensor {}'.format(name, tuple(src.shape)))
    out = torch.empty((n, 2 * c), dtype=torch.int64, device=src.device)
    check(fn[name](_ptr(src), n, pixels, c, _ptr(out), _stream()), name)
    return out


# ---------------------------------------------------------------------------------------------- CowMask
_COW_WORKSPACE = {}


def _f64_on(t, device, shape, what):
    """numpy / tensor -> contiguous float64 tensor of `shape` on `device`"""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
    if tuple(t.shape) != tuple(shape):
        raise ValueError('cowmask: {} has shape {}, {} expected'.format(what, tuple(t.shape), tuple(shape)))
    if not t.is_cuda:
        t = t.to(torch.float64).contiguous().pin_memory()          # as ranges_to_device: a copy the host does not wait for
    return t.to(device=device, dtype=torch.float64, non_blocking=True).contiguous()


def cowmask(noise, taps, thresh_factor, out=None, stats=None):
    """noise f32 CUDA (N,1,H,W) or (N,H,W); taps float64 (N, 2R+1), one row of 1-D blur weights per sample; thresh_factor float64
    (N,) -> f32 (N,1,H,W) mask = [s <= mean(s) + std(s) * thresh_factor], s = the noise blurred with the taps along x and along y
    under zero padding, everything in fp64 (csrc/cowmask.hip). `taps` and `thresh_factor` may be numpy arrays (copied to the
    device). `stats`: optional float64 CUDA (N, 2) that receives each sample's mean and std. Deterministic; R <= 128."""
    _need_cuda(noise, out, stats)
    if noise.dtype != torch.float32 or noise.dim() not in (3, 4) or (noise.dim() == 4 and noise.shape[1] != 1):
        raise TypeError('cowmask: noise must be a float32 (N,1,H,W) or (N,H,W) tensor')
    noise = noise.contiguous()
    n, h, w = int(noise.shape[0]), int(noise.shape[-2]), int(noise.shape[-1])
    k = int(taps.shape[-1])
    if k < 1 or k % 2 == 0:
        raise ValueError('cowmask: taps must have an odd number of columns (2R+1), got {}'.format(k))
    radius = (k - 1) // 2
    if radius > 128:
        raise ValueError('cowmask: a radius of {} is not built (at most 128)'.format(radius))
    taps = _f64_on(taps, noise.device, (n, k), 'taps')
    thresh_factor = _f64_on(thresh_factor, noise.device, (n,), 'thresh_factor')
    if out is None:
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=noise.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, 1, h, w):
        raise TypeError('cowmask: out must be a contiguous float32 tensor of shape {}'.format((n, 1, h, w)))
    if stats is not None and (stats.dtype != torch.float64 or not stats.is_contiguous() or tuple(stats.shape) != (n, 2)):
        raise TypeError('cowmask: stats must be a contiguous float64 tensor of shape {}'.format((n, 2)))
    need = int(fn['cms_cowmask_workspace_bytes'](n, h, w))
    if need == 0:
        raise ValueError('cowmask: {} x {} x {} is more than the kernel takes'.format(n, h, w))
    # one workspace per device, grown on demand: launches are stream-ordered, and a trainer makes its masks on one stream
    key = str(noise.device)
    ws = _COW_WORKSPACE.get(key)
    if ws is None or ws.numel() < need:
        ws = _COW_WORKSPACE[key] = torch.empty(need, dtype=torch.uint8, device=noise.device)
    check(fn['cms_cowmask'](_ptr(noise), _ptr(taps), _ptr(thresh_factor), n, h, w, radius, _ptr(out), _ptr(stats), _ptr(ws),
                            C.c_size_t(ws.numel()), _stream()), 'cms_cowmask')
    return out


# ---------------------------------------------------------------------------------------------- ClassMix
def _classmix_keys(keys, n, c, device):
    """host array / tensor of (n, c) keys -> contiguous float64 tensor on `device`; shape and (on the host) finiteness checked
    before the GPU is touched"""
    if torch.is_tensor(keys):
        if tuple(keys.shape) != (n, c):
            raise ValueError('classmix_mask: keys have shape {}, {} expected'.format(tuple(keys.shape), (n, c)))
        if keys.is_cuda:
            if keys.dtype != torch.float64:
                raise TypeError('classmix_mask: device keys must be float64, got {}'.format(keys.dtype))
            return keys.contiguous()
        keys = keys.detach().numpy()
    keys = np.ascontiguousarray(keys, dtype=np.float64)
    if keys.shape != (n, c):
        raise ValueError('classmix_mask: keys have shape {}, {} expected'.format(keys.shape, (n, c)))
    if not np.all(np.isfinite(keys)):
        raise ValueError('classmix_mask: keys must be finite')
    return None if device is None else _f64_on(keys, device, (n, c), 'keys')


def classmix_mask(logits, keys, out_size, align_corners=True, valid=None, out=None, pred_out=None, sets_out=None):
    """
    The ClassMix mask of a batch (csrc/classmix.hip): logits (N,C,h,w) CUDA (converted to fp32 as tta_vote does), keys float64 (N,C)
    -- a host array or a device tensor --, valid optional f32 (N,1,H,W) / (N,H,W). Per sample: pred = the argmax of the logits
    upsampled to `out_size` (bit for bit tta_vote's single-view prediction), present = the classes predicted at some pixel with
    valid != 0, chosen = the ceil(|present| / 2) present classes with the smallest (key, class index), mask = 1 where valid != 0 and
    pred is chosen. Returns the f32 (N,1,H,W) mask (`out` when given). `pred_out`: a contiguous uint8 (N,H,W) tensor that receives
    pred; `sets_out`: a contiguous int64 (N,2) tensor that receives [present, chosen] as 64-bit sets (bit 63 is the sign bit). Two
    launches on the current stream, no host synchronisation; the same inputs give the same bits.
    """
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise TypeError('classmix_mask: logits must be an (N,C,h,w) tensor')
    n, c, h, w = (int(s) for s in logits.shape)
    if min(n, c, h, w) < 1:
        raise ValueError('classmix_mask: empty logits {}'.format(tuple(logits.shape)))
    if c > 64:
        raise ValueError('classmix_mask: 1 <= num_classes <= 64, got {}'.format(c))
    H, W = _size2(out_size, 'classmix_mask: out_size')
    _classmix_keys(keys, n, c, None)                       # shape and finiteness, before the GPU is touched
    _need_cuda(logits, valid, out, pred_out, sets_out)
    if n > 65535 or n * H * W > 2 ** 31 - 1:
        raise ValueError('classmix_mask: more than 65535 samples or 2^31 - 1 output pixels')
    logits = _f32c(logits)
    dev = logits.device
    keys = _classmix_keys(keys, n, c, dev)
    if valid is not None:
        if valid.dim() == 4 and valid.shape[1] == 1:
            valid = valid[:, 0]
        if tuple(valid.shape) != (n, H, W):
            raise ValueError('classmix_mask: valid has shape {}, {} expected'.format(tuple(valid.shape), (n, H, W)))
        valid = _f32c(valid)
    if out is None:
        out = torch.empty((n, 1, H, W), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, 1, H, W):
        raise TypeError('classmix_mask: out must be a contiguous float32 tensor of shape {}'.format((n, 1, H, W)))
    if pred_out is not None and (pred_out.dtype != torch.uint8 or not pred_out.is_contiguous() or tuple(pred_out.shape) != (n, H, W)):
        raise TypeError('classmix_mask: pred_out must be a contiguous uint8 tensor of shape {}'.format((n, H, W)))
    if sets_out is not None and (sets_out.dtype != torch.int64 or not sets_out.is_contiguous() or tuple(sets_out.shape) != (n, 2)):
        raise TypeError('classmix_mask: sets_out must be a contiguous int64 tensor of shape {}'.format((n, 2)))
    d = _lib.ClassMixDesc()
    d.logits, d.valid, d.keys = logits.data_ptr(), (valid.data_ptr() if valid is not None else None), keys.data_ptr()
    d.n, d.c, d.h, d.w, d.H, d.W, d.align_corners = n, c, h, w, H, W, int(bool(align_corners))
    d.mask_out = out.data_ptr()
    d.pred_out = pred_out.data_ptr() if pred_out is not None else None
    sets = None
    if sets_out is not None:
        # the kernel writes (n) words each: a (2, n) staging tensor, transposed into the caller's (n, 2)
        sets = torch.empty((2, n), dtype=torch.int64, device=dev)
        d.present_out, d.chosen_out = sets[0].data_ptr(), sets[1].data_ptr()
    need = int(fn['cms_classmix_workspace_bytes'](n, H, W))
    if need == 0:
        raise ValueError('classmix_mask: {} x {} x {} is more than the kernel takes'.format(n, H, W))
    ws = _workspace_bytes(need, dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(fn['cms_classmix'](C.byref(d), _stream()), 'cms_classmix')
    if sets is not None:
        sets_out.copy_(sets.t())
    return out


# ---------------------------------------------------------------------------------------------- cross pseudo supervision
def _cps_map(name, t, n, H, W):
    """an optional f32 (N,1,H,W) / (N,H,W) map -> contiguous f32 (N,H,W)"""
    if t is None:
        return None
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != (n, H, W):
        raise ValueError('cps_labels: {} has shape {}, {} expected'.format(name, tuple(t.shape), (n, H, W)))
    return _f32c(t)


def cps_labels(l0_a, l1_a, l0_b, l1_b, out_size, ranges=None, mask=None, invert=True, um0=None, um1=None, conf_thresh=0.0,
               align_corners=True, labels_out=None, stats_out=None):
    """
    The hard pseudo-labels two networks give each other on a CutMix-ed pair (csrc/cps.hip): four (N,C,h,w) CUDA logit tensors
    (converted to fp32 as the loss kernels do), exactly one of `ranges` (int32 (N,nb,4), read under `invert` as the consistency kernels
    read it) and `mask` (f32 (N,1,H,W) / (N,H,W), >= 0.5 takes image 1), optional validity maps um0 / um1. Per pixel and network k:
    u_k = the upsampled logits of image 1 where the mask says so, else of image 0; pred_k = argmax u_k; label_k = pred_k where the
    pixel's validity map is >= 0.5 and (conf_thresh <= 0 or max softmax(u_k) >= conf_thresh), else 255. Returns (label_a, label_b,
    stats): two uint8 (N,H,W) maps -- `labels_out`, a pair of contiguous uint8 (N,H,W) tensors, when given -- and int64[4]
    = [valid pixels, labels kept in a, labels kept in b, valid pixels where the predictions agree] (`stats_out` when given). One
    launch on the current stream, no host synchronisation; the same inputs give the same bits whatever the outputs held.
    """
    logits = (l0_a, l1_a, l0_b, l1_b)
    if not all(torch.is_tensor(t) and t.dim() == 4 for t in logits):
        raise TypeError('cps_labels: the logits must be four (N,C,h,w) tensors')
    if any(tuple(t.shape) != tuple(l0_a.shape) for t in logits):
        raise ValueError('cps_labels: the four logit tensors differ in shape')
    n, c, h, w = (int(s) for s in l0_a.shape)
    if min(n, c, h, w) < 1:
        raise ValueError('cps_labels: empty logits {}'.format(tuple(l0_a.shape)))
    if c > 64:
        raise ValueError('cps_labels: 1 <= num_classes <= 64, got {}'.format(c))
    H, W = _size2(out_size, 'cps_labels: out_size')
    if h > H or w > W:
        raise ValueError('cps_labels: logits of {} x {} are larger than the output {} x {}'.format(h, w, H, W))
    if (ranges is None) == (mask is None):
        raise ValueError('cps_labels: give exactly one of ranges / mask')
    _need_cuda(l0_a, l1_a, l0_b, l1_b, ranges, mask, um0, um1, stats_out, *(labels_out or ()))
    if n > 65535 or n * H * W > 2 ** 31 - 1:
        raise ValueError('cps_labels: more than 65535 samples or 2^31 - 1 output pixels')
    l0_a, l1_a, l0_b, l1_b = (_f32c(t) for t in logits)
    dev = l0_a.device
    if ranges is not None:
        if ranges.dtype != torch.int32 or ranges.dim() != 3 or ranges.shape[0] != n or ranges.shape[2] != 4:
            raise ValueError('cps_labels: ranges must be an int32 ({}, n_boxes, 4) tensor'.format(n))
        ranges = _nonempty_ranges(ranges).contiguous()
    mask, um0, um1 = _cps_map('mask', mask, n, H, W), _cps_map('um0', um0, n, H, W), _cps_map('um1', um1, n, H, W)
    if labels_out is None:
        # two allocations: each map starts aligned, whatever N * H * W is, and gets the kernel's 4-byte stores
        labels_out = (torch.empty((n, H, W), dtype=torch.uint8, device=dev), torch.empty((n, H, W), dtype=torch.uint8, device=dev))
    elif len(labels_out) != 2 or any(t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (n, H, W) for t in labels_out):
        raise TypeError('cps_labels: labels_out must be a pair of contiguous uint8 tensors of shape {}'.format((n, H, W)))
    if stats_out is None:
        stats_out = torch.empty(4, dtype=torch.int64, device=dev)
    elif stats_out.dtype != torch.int64 or not stats_out.is_contiguous() or tuple(stats_out.shape) != (4,):
        raise TypeError('cps_labels: stats_out must be a contiguous int64 tensor of shape (4,)')
    d = _lib.CpsDesc()
    d.l0_a, d.l1_a, d.l0_b, d.l1_b = l0_a.data_ptr(), l1_a.data_ptr(), l0_b.data_ptr(), l1_b.data_ptr()
    d.ranges = ranges.data_ptr() if ranges is not None else None
    d.mask = mask.data_ptr() if mask is not None else None
    d.um0 = um0.data_ptr() if um0 is not None else None
    d.um1 = um1.data_ptr() if um1 is not None else None
    d.n, d.c, d.h, d.w, d.H, d.W, d.align_corners = n, c, h, w, H, W, int(bool(align_corners))
    d.n_boxes = int(ranges.shape[1]) if ranges is not None else 0
    d.invert = int(bool(invert))
    d.conf_thresh = float(conf_thresh)
    d.label_a, d.label_b, d.stats = labels_out[0].data_ptr(), labels_out[1].data_ptr(), stats_out.data_ptr()
    check(fn['cms_cps_labels'](C.byref(d), _stream()), 'cms_cps_labels')
    return labels_out[0], labels_out[1], stats_out


# ---------------------------------------------------------------------------------------------- boundary scores
_BOUNDARY_WIDTHS = {}       # (device, shape, bytes) -> the int32 table on the device: an evaluation asks for the same few tables


def _boundary_widths_on(wd, device):
    """The device copy of a validated (N,K) int32 table. Tables are small, read-only and repeat from batch to batch, so a table seen
    before costs no upload (an upload from pageable memory makes the host wait for the stream)."""
    key = (str(device), wd.shape, wd.tobytes())
    t = _BOUNDARY_WIDTHS.get(key)
    if t is None:
        if len(_BOUNDARY_WIDTHS) >= 256:
            _BOUNDARY_WIDTHS.clear()
        t = _BOUNDARY_WIDTHS[key] = torch.from_numpy(wd.copy()).to(device)
    return t


def _boundary_widths(widths, n):
    """-> int32 (n, K) host array; a list of K ints is broadcast over the batch"""
    w = np.asarray(widths)
    if w.dtype.kind not in 'iu' or w.ndim not in (1, 2) or w.size == 0:
        raise TypeError('boundary_confusion: widths must be K integers or an (N,K) integer array, got {!r}'.format(widths))
    if w.ndim == 1:
        w = np.broadcast_to(w[None, :], (n, w.shape[0]))
    if w.shape[0] != n or not 1 <= w.shape[1] <= 4:
        raise ValueError('boundary_confusion: widths have shape {}, ({}, 1..4) expected'.format(tuple(w.shape), n))
    if int(w.min()) < 1 or int(w.max()) > 254:
        raise ValueError('boundary_confusion: widths must lie in 1..254, got {}..{}'.format(int(w.min()), int(w.max())))
    return np.ascontiguousarray(w, dtype=np.int32)


def boundary_confusion(truth, pred, num_classes, widths, ignore_index=255, bcm=None, tcm=None, want_dist=False):
    """
    The counts behind Boundary IoU and trimap IoU (csrc/boundary.hip): truth, pred uint8 CUDA (N,H,W) [or (H,W)], `widths` K <= 4
    band widths in pixels (a list, the same for every sample, or an (N,K) array). With D the Chebyshev distance of a pixel to the
    nearest pixel of another value, void pixel (truth == ignore_index) or array edge, in the truth map (D_T) and in the prediction
    with the void pixels blanked (D_P): bcm[j] (C+1,C+1) += 1 at [D_T <= d ? truth : C, D_P <= d ? pred : C] per non-void pixel, tcm[j]
    (C,C) += 1 at [truth, pred] per non-void pixel with D_T <= d. Returns (bcm (K,C+1,C+1), tcm (K,C,C), (dist_truth, dist_pred) |
    None): int64 matrices (accumulated into when given) and, with `want_dist`, the uint8 maps min(D, 255), 0 at void pixels. The
    number of launches depends on C and K only, and nothing waits for the device but the upload of a widths table not seen before.
    """
    if not torch.is_tensor(truth) or not torch.is_tensor(pred):
        raise TypeError('boundary_confusion: truth and pred must be tensors')
    if truth.dtype != torch.uint8 or pred.dtype != torch.uint8:
        raise TypeError('boundary_confusion: uint8 maps required')
    if truth.dim() not in (2, 3) or truth.shape != pred.shape:
        raise ValueError('boundary_confusion: truth and pred must be (N,H,W) or (H,W) maps of one shape, got {} and {}'.format(
            tuple(truth.shape), tuple(pred.shape)))
    n = int(truth.shape[0]) if truth.dim() == 3 else 1
    h, w = int(truth.shape[-2]), int(truth.shape[-1])
    c = int(num_classes)
    if not 1 <= c <= 64:
        raise ValueError('boundary_confusion: 1 <= num_classes <= 64, got {}'.format(c))
    if min(n, h, w) < 1 or n * h * w > 2 ** 31 - 1:
        raise ValueError('boundary_confusion: {} x {} x {} maps: empty, or more than 2^31 - 1 pixels'.format(n, h, w))
    wd = _boundary_widths(widths, n)
    k = int(wd.shape[1])
    for name, m, shape in (('bcm', bcm, (k, c + 1, c + 1)), ('tcm', tcm, (k, c, c))):
        if m is not None and (not torch.is_tensor(m) or m.dtype != torch.int64 or tuple(m.shape) != shape or not m.is_contiguous()):
            raise TypeError('boundary_confusion: {} must be a contiguous int64 tensor of shape {}'.format(name, shape))
    _need_cuda(truth, pred, bcm, tcm)
    dev = truth.device
    truth, pred = truth.contiguous(), pred.contiguous()
    if bcm is None:
        bcm = torch.zeros((k, c + 1, c + 1), dtype=torch.int64, device=dev)
    if tcm is None:
        tcm = torch.zeros((k, c, c), dtype=torch.int64, device=dev)
    wd_dev = _boundary_widths_on(wd, dev)
    dist = None
    if want_dist:
        dist = (torch.empty_like(truth), torch.empty_like(truth))
    d = _lib.BoundaryDesc()
    d.truth, d.pred, d.widths = truth.data_ptr(), pred.data_ptr(), wd_dev.data_ptr()
    d.n, d.h, d.w, d.num_classes, d.k = n, h, w, c, k
    d.ignore_index = -1 if ignore_index is None else int(ignore_index)
    d.bcm, d.tcm = bcm.data_ptr(), tcm.data_ptr()
    if dist is not None:
        d.dist_truth, d.dist_pred = dist[0].data_ptr(), dist[1].data_ptr()
    need = int(fn['cms_boundary_workspace_bytes'](n, h, w))
    ws = _workspace_bytes(need, dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(fn['cms_boundary_confusion'](C.byref(d), _stream()), 'cms_boundary_confusion')
    return bcm, tcm, dist


# ---------------------------------------------------------------------------------------------- surface distances
def surface_distances(truth, pred, num_classes, ignore_index=255, want_maps=False):
    """
    What HD, HD95 and ASSD follow from (csrc/surface.hip): truth, pred uint8 CUDA (N,H,W) [or (H,W)]. Per image and class, with G the
    class mask of the truth, S that of the prediction with the void pixels (truth == ignore_index) blanked and the surface of a mask
    its pixels with a 4-neighbour outside it: d2 is the exact squared Euclidean distance from a surface pixel of one mask to the
    nearest surface pixel of the other. Returns (stats int64 (N,C,6) = [|dS|, |dG|, max d2 over dS, max d2 over dG, a[lo], a[hi]] with a
    the sorted pooled d2 and lo, hi the ranks behind numpy.percentile(., 95); sums float64 (N,C,2) = the two directed sums of sqrt(d2);
    with `want_maps` (d2_pred, d2_truth) int32 (N,H,W), -1 off the surfaces, else None). A pair with an empty G or S is not scored:
    its counts, -1 in the other four and 0.0. A fixed number of launches; nothing waits for the device.
    """
    if not torch.is_tensor(truth) or not torch.is_tensor(pred):
        raise TypeError('surface_distances: truth and pred must be tensors')
    if truth.dtype != torch.uint8 or pred.dtype != torch.uint8:
        raise TypeError('surface_distances: uint8 maps required')
    if truth.dim() not in (2, 3) or truth.shape != pred.shape:
        raise ValueError('surface_distances: truth and pred must be (N,H,W) or (H,W) maps of one shape, got {} and {}'.format(
            tuple(truth.shape), tuple(pred.shape)))
    n = int(truth.shape[0]) if truth.dim() == 3 else 1
    h, w = int(truth.shape[-2]), int(truth.shape[-1])
    c = int(num_classes)
    if not 1 <= c <= 64:
        raise ValueError('surface_distances: 1 <= num_classes <= 64, got {}'.format(c))
    if min(n, h, w) < 1 or max(h, w) > 16384 or n * h * w > 2 ** 31 - 1:
        raise ValueError('surface_distances: {} x {} x {} maps: empty, a side above 16384, or more than 2^31 - 1 pixels'.format(n, h, w))
    _need_cuda(truth, pred)
    dev = truth.device
    truth, pred = truth.contiguous(), pred.contiguous()
    stats = torch.empty((n, c, 6), dtype=torch.int64, device=dev)
    sums = torch.empty((n, c, 2), dtype=torch.float64, device=dev)
    maps = None
    if want_maps:
        maps = (torch.empty((n, h, w), dtype=torch.int32, device=dev), torch.empty((n, h, w), dtype=torch.int32, device=dev))
    d = _lib.SurfaceDesc()
    d.truth, d.pred = truth.data_ptr(), pred.data_ptr()
    d.n, d.h, d.w, d.num_classes = n, h, w, c
    d.ignore_index = -1 if ignore_index is None else int(ignore_index)
    d.stats, d.sums = stats.data_ptr(), sums.data_ptr()
    if maps is not None:
        d.d2_pred, d.d2_truth = maps[0].data_ptr(), maps[1].data_ptr()
    ws = _workspace_bytes(int(fn['cms_surface_workspace_bytes'](n, h, w, c)), dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(fn['cms_surface_distances'](C.byref(d), _stream()), 'cms_surface_distances')
    if maps is not None and truth.dim() == 2:
        maps = (maps[0][0], maps[1][0])
    return stats, sums, maps


# ---------------------------------------------------------------------------------------------- fp64 FFT / patch distances
_TWIDDLES = {}


def fft_twiddles(n, device):
    """exp(-2 pi i k / n), k < n / 2, built on the host in float64 and cached per (length, device): complex128 CUDA (n / 2,)"""
    key = (int(n), str(device))
    if key not in _TWIDDLES:
        k = np.arange(n // 2, dtype=np.float64)
        _TWIDDLES[key] = torch.from_numpy(np.exp(-2j * np.pi * k / n).astype(np.complex128)).to(device)
    return _TWIDDLES[key]


def fft_size(n):
    """the FFT length that serves a padded extent n: the smallest power of two >= max(8, n), at most 4096"""
    n = int(n)
    size = 8
    while size < n:
        size *= 2
    if size > 4096:
        raise ValueError('fft_size: an extent of {} needs an FFT longer than 4096, which is not built'.format(n))
    return size


def fft2(x, inverse=False):
    """2-D FFT over the last two axes of a contiguous complex128 CUDA (B, FH, FW) tensor, IN PLACE (csrc/fft.hip); power-of-two
    lengths 8 ... 4096; the inverse is scaled by 1 / (FH * FW). Returns x."""
    _need_cuda(x)
    if x.dtype != torch.complex128 or x.dim() != 3 or not x.is_contiguous():
        raise TypeError('fft2: a contiguous complex128 (B, FH, FW) tensor is required')
    b, fh, fw = (int(v) for v in x.shape)
    check(fn['cms_fft2'](_ptr(x), b, fh, fw, int(bool(inverse)), _ptr(fft_twiddles(fh, x.device)), _ptr(fft_twiddles(fw, x.device)),
                         _stream()), 'cms_fft2')
    return x


def pd_load_image(pool_img, entry, patch_shape, fft_shape, planes, sq=None):
    """pool entry (a _lib.StageEntry on the host) -> planes complex128 (3, FH, FW), sq int64 (Hs + ph - 1, Ws + pw - 1)"""
    _need_cuda(pool_img, planes, sq)
    check(fn['cms_pd_load_image'](_ptr(pool_img), C.byref(entry), int(patch_shape[0]), int(patch_shape[1]), int(fft_shape[0]),
                                  int(fft_shape[1]), _ptr(planes), _ptr(sq), _stream()), 'cms_pd_load_image')


def pd_load_patches(pool_img, patches, n, patch_shape, fft_shape, planes):
    """patches: CUDA uint8 table of n cms_pd_patch -> planes complex128 ((n + 1) // 2, 3, FH, FW), flipped and packed in pairs"""
    _need_cuda(pool_img, patches, planes)
    check(fn['cms_pd_load_patches'](_ptr(pool_img), _ptr(patches), int(n), int(patch_shape[0]), int(patch_shape[1]), int(fft_shape[0]),
                                    int(fft_shape[1]), _ptr(planes), _stream()), 'cms_pd_load_patches')


def pd_patch_sqdiff(pool_img, a, b, n, patch_shape):
    """int64 (n,): sum over each patch of (a - b)^2, or of a^2 with b None"""
    _need_cuda(pool_img, a, b)
    out = torch.empty((int(n),), dtype=torch.int64, device=pool_img.device)
    check(fn['cms_pd_patch_sqdiff'](_ptr(pool_img), _ptr(a), _ptr(b), int(n), int(patch_shape[0]), int(patch_shape[1]), _ptr(out),
                                    _stream()), 'cms_pd_patch_sqdiff')
    return out


def pd_spectrum_product(f_img, f_pairs, out):
    _need_cuda(f_img, f_pairs, out)
    check(fn['cms_pd_spectrum_product'](_ptr(f_img), _ptr(f_pairs), int(f_pairs.shape[0]), int(f_img.shape[-2]), int(f_img.shape[-1]),
                                        _ptr(out), _stream()), 'cms_pd_spectrum_product')
    return out


def pd_finish(corr, p2, q2, residual_bits, d2=None, keys=None):
    """corr complex128 (pairs, FH, FW), p2 int64 (H, W), q2 int64 (n,) -> d2 (n, H, W) and / or keys (n, H * W); residual_bits:
    int64 (1,), max-accumulates the bit pattern of the largest |re - rint(re)|"""
    _need_cuda(corr, p2, q2, residual_bits, d2, keys)
    check(fn['cms_pd_finish'](_ptr(corr), _ptr(p2), _ptr(q2), int(q2.shape[0]), int(p2.shape[0]), int(p2.shape[1]), int(corr.shape[-2]),
                              int(corr.shape[-1]), _ptr(d2), _ptr(keys), _ptr(residual_bits), _stream()), 'cms_pd_finish')


def _int64_buffer(what, t, numel, device):
    """a caller's int64 buffer of at least `numel` elements, or a fresh one (the kernels initialise nothing they do not write)"""
    if t is None:
        return torch.empty((max(int(numel), 1),), dtype=torch.int64, device=device)
    _need_cuda(t)
    if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < numel:
        raise TypeError('{}: a contiguous int64 CUDA tensor of at least {} elements is required'.format(what, numel))
    return t


def pd_box_sum(x, box, out=None, work=None):
    """int32 or int64 CUDA plane (hp, wp) -> int64 (hp - bh + 1, wp - bw + 1): the exact sum of every bh x bw window, by two
    running-sum passes (csrc/patchdist.hip). `out` and `work` ((hp - bh + 1) * wp int64) may be given; neither needs a value."""
    _need_cuda(x)
    if x.dtype not in (torch.int32, torch.int64) or x.dim() != 2 or not x.is_contiguous():
        raise TypeError('pd_box_sum: a contiguous int32 or int64 (H, W) tensor is required')
    hp, wp, bh, bw = int(x.shape[0]), int(x.shape[1]), int(box[0]), int(box[1])
    if bh < 1 or bw < 1 or bh > hp or bw > wp:
        raise ValueError('pd_box_sum: a box of {} x {} does not fit a plane of {} x {}'.format(bh, bw, hp, wp))
    ho, wo = hp - bh + 1, wp - bw + 1
    out = _int64_buffer('pd_box_sum: out', out, ho * wo, x.device)
    work = _int64_buffer('pd_box_sum: work', work, ho * wp, x.device)
    check(fn['cms_pd_box_sum'](_ptr(x), int(x.dtype == torch.int64), hp, wp, bh, bw, _ptr(work), _ptr(out), _stream()), 'cms_pd_box_sum')
    return out[:ho * wo].view(ho, wo)


def pd_neighbour_workspace(hs, ws, patch_shape):
    """int64 elements of the workspace of pd_neighbour_maps"""
    return (int(fn['cms_pd_neighbour_workspace_bytes'](int(hs), int(ws), int(patch_shape[0]), int(patch_shape[1]))) + 7) // 8


def pd_neighbour_maps(pool_img, entry, patch_shape, out=None, work=None):
    """pool entry (a _lib.StageEntry on the host) -> int64 (4, Hs, Ws): the exact squared distance, in grey levels, of the patch
    centred on each pixel to the patches centred on its left, right, upper and lower neighbour"""
    _need_cuda(pool_img)
    hs, ws = int(entry.hs), int(entry.ws)
    out = _int64_buffer('pd_neighbour_maps: out', out, 4 * hs * ws, pool_img.device)
    work = _int64_buffer('pd_neighbour_maps: work', work, pd_neighbour_workspace(hs, ws, patch_shape), pool_img.device)
    check(fn['cms_pd_neighbour_maps'](_ptr(pool_img), C.byref(entry), int(patch_shape[0]), int(patch_shape[1]), _ptr(work), _ptr(out),
                                      _stream()), 'cms_pd_neighbour_maps')
    return out[:4 * hs * ws].view(4, hs, ws)


def select_k_smallest(keys, k, mask=None, labels=None, cls=None, inter=False):
    """
    The k smallest candidate keys of each row of `keys` (int64 CUDA (N, M), non-negative, distinct within a row), by a radix select
    on the device; the <= k survivors are then sorted. Candidates: `mask` (N, M) bool / uint8, or `labels` uint8 (M,) with `cls`
    int32 (N,): label == cls[row], or with `inter` label != cls[row] and label != 255.
    Returns (sorted int64 (N, k) with INT64_MAX past each row's count, int32 (N,) counts).
    """
    _need_cuda(keys, mask, labels, cls)
    if keys.dtype != torch.int64 or keys.dim() != 2 or not keys.is_contiguous():
        raise TypeError('select_k_smallest: keys must be a contiguous int64 (N, M) tensor')
    n, m = int(keys.shape[0]), int(keys.shape[1])
    k = int(k)
    if k < 1:
        raise ValueError('select_k_smallest: k must be positive')
    if mask is not None:
        if labels is not None or cls is not None:
            raise ValueError('select_k_smallest: give a mask, or labels and cls')
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (n, m):
            raise TypeError('select_k_smallest: mask must be bool / uint8 of the shape of keys')
        mask, mode = mask.contiguous(), 0
    else:
        if labels is None or cls is None:
            raise ValueError('select_k_smallest: give a mask, or labels and cls')
        if labels.dtype != torch.uint8 or labels.numel() != m or cls.dtype != torch.int32 or cls.numel() != n:
            raise TypeError('select_k_smallest: labels uint8 (M,) and cls int32 (N,) required')
        labels, cls, mode = labels.contiguous(), cls.contiguous(), 2 if inter else 1
    out = torch.empty((n, k), dtype=torch.int64, device=keys.device)
    count = torch.empty((n,), dtype=torch.int32, device=keys.device)
    nbytes = int(fn['cms_select_workspace_bytes'](n))
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device=keys.device)
    check(fn['cms_select_k_smallest'](_ptr(keys), _ptr(mask), _ptr(labels), _ptr(cls), mode, n, m, k, _ptr(out), _ptr(count), _ptr(ws),
                                      nbytes, _stream()), 'cms_select_k_smallest')
    return torch.sort(out, dim=1).values, torch.clamp(count, max=k)


# ---------------------------------------------------------------------------------------------- BatchNorm (batch stats)
def _world(group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


_BN_WHAT = {'reduce': _lib.BN_REDUCE, 'finalize': _lib.BN_FINALIZE, 'apply': _lib.BN_APPLY, 'reduce_bwd': _lib.BN_REDUCE_BWD,
            'bwd_apply': _lib.BN_BWD_APPLY, 'count': _lib.BN_COUNT, 'stats': _lib.BN_STATS, 'finalize_tiles': _lib.BN_FINALIZE_TILES,
            'sums_tiles': _lib.BN_BWD_SUMS_TILES}
_BN_DTYPE = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, None: _lib.BF16}      # (None: kinds that touch no activation)


def _bn_desc(what, c=0, dtype=None, n_pixels=0, count=0.0, relu=False, eps=1e-5, momentum=0.1, groups=1, tile_rows=0, **t):
    """The cms_bn_op of one launch (arguments: bn_op). It is host time of the eager U-Net / DeepLab v3+ head passes: the struct
    starts zeroed and only what is not zero is set."""
    d = _lib.BnOp()
    d.what = _BN_WHAT[what]
    if dtype not in _BN_DTYPE:
        raise TypeError('unsupported dtype {}'.format(dtype))
    d.dtype = _BN_DTYPE[dtype]
    d.c, d.groups, d.n_pixels = int(c), int(groups), int(n_pixels)
    d.eps, d.momentum = float(eps), float(momentum)
    if relu:
        d.relu = 1
    if count:
        d.count = float(count)
    if tile_rows:
        d.tile_rows = int(tile_rows)
    for k, v in t.items():
        if v is not None:
            setattr(d, k, v.data_ptr())
    return d


def _bn_run(d):
    check(fn['cms_bn_run'](C.byref(d), _stream()), 'cms_bn_run')


class _BatchNormActFn(torch.autograd.Function):
    """relu(batch_norm(x) (+ res)) on NHWC tensors with batch statistics (csrc/bn.hip); under torch.distributed the
    statistics are all-reduced between the two passes of either direction (SyncBN). `groups`: the batch
    is that many equal runs of samples normalised separately (one launch for what the reference does in separate passes)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, running_mean, running_var, momentum, eps, relu, group, groups):
        n_pix = x.numel() // x.shape[-1]
        c = int(x.shape[-1])
        dev = x.device
        mean, rstd, scale, shift = (torch.empty(groups * c, dtype=torch.float32, device=dev) for _ in range(4))
        ws = bn_workspace(n_pix, c, dev, groups)
        world = _world(group)
        if world > 1:
            # SyncBN, sample groups included (round 4): every group's (sum x, sum x^2) summed over the ranks in ONE all-reduce of
            # [G][2][C] doubles, then finalised group by group, in order (the running statistics move once per group, as in the
            # reference's separate passes); count = the group's pixels on ALL ranks
            stats = torch.empty(groups * 2 * c, dtype=torch.float64, device=dev)
            _bn_run(_bn_desc('reduce', c=c, dtype=x.dtype, n_pixels=n_pix, groups=groups, x=x, sums=stats, ws=ws))
            _allreduce_sum(stats, group)
            count = float(n_pix // groups) * world       # (equal shards: the per-GPU batch is fixed under weak scaling)
            for g in range(groups):
                sl = slice(g * c, (g + 1) * c)
                _bn_run(_bn_desc('finalize', c=c, count=count, eps=eps, momentum=momentum, sums=stats[g * 2 * c:(g + 1) * 2 * c],
                                 gamma=gamma, beta=beta, mean=mean[sl], rstd=rstd[sl], scale=scale[sl], shift=shift[sl],
                                 running_mean=running_mean, running_var=running_var))
        else:                                  # statistics and their finalisation in ONE launch
            count = float(n_pix // groups)
            _bn_run(_bn_desc('stats', c=c, dtype=x.dtype, n_pixels=n_pix, groups=groups, eps=eps, momentum=momentum, x=x, ws=ws,
                             gamma=gamma, beta=beta, mean=mean, rstd=rstd, scale=scale, shift=shift, running_mean=running_mean,
                             running_var=running_var))
        y = torch.empty_like(x)
        _bn_run(_bn_desc('apply', c=c, dtype=x.dtype, n_pixels=n_pix, groups=groups, relu=relu, x=x, res=res, y=y, scale=scale,
                         shift=shift))
        ctx.save_for_backward(x, y if relu else None, mean, rstd, gamma, ws)
        ctx.meta = (n_pix, c, count, group, res is not None, gamma is not None and gamma.requires_grad,
                    beta is not None and beta.requires_grad, groups)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd, gamma, ws = ctx.saved_tensors
        n_pix, c, count, group, has_res, want_g, want_b, groups = ctx.meta
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        sums = torch.empty(groups * 2 * c, dtype=torch.float64, device=x.device)
        _bn_run(_bn_desc('reduce_bwd', c=c, dtype=x.dtype, n_pixels=n_pix, groups=groups, x=x, dy=dy, y=y, mean=mean, rstd=rstd,
                         sums=sums, ws=ws))
        local = sums
        if _world(group) > 1:
            local = sums.clone()                 # parameter gradients stay local (the arena all-reduce sums them)
            _allreduce_sum(sums, group)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if has_res else None
        _bn_run(_bn_desc('bwd_apply', c=c, dtype=x.dtype, n_pixels=n_pix, groups=groups, count=count, x=x, dy=dy, y=y, dx=dx,
                         dres=dres, mean=mean, rstd=rstd, gamma=gamma, sums=sums))
        local = local.view(groups, 2, c).sum(0)    # the groups' passes add into the same parameter gradients
        dgamma = local[1].float() if want_g else None
        dbeta = local[0].float() if want_b else None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None


class _FrozenBnActFn(torch.autograd.Function):
    """relu(x * scale + shift (+ res)) on contiguous NHWC tensors, scale / shift fp32 [C] WITHOUT gradient (an eval-mode BatchNorm whose
    affine does not train: the teacher of the VAT trainer): one launch forward (the 'apply' kind), one backward (cms_frozen_bn_act_bwd)."""

    @staticmethod
    def forward(ctx, x, scale, shift, res, relu):
        n_pix = x.numel() // x.shape[-1]
        c = int(x.shape[-1])
        y = torch.empty_like(x)
        _bn_run(_bn_desc('apply', c=c, dtype=x.dtype, n_pixels=n_pix, relu=relu, x=x, res=res, y=y, scale=scale, shift=shift))
        ctx.save_for_backward(scale, y if relu else None)
        ctx.geo = (n_pix, c, res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        scale, y = ctx.saved_tensors
        n_pix, c, has_res = ctx.geo
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx = torch.empty_like(dy)
        dres = torch.empty_like(dy) if (has_res and ctx.needs_input_grad[3]) else None
        check(fn['cms_frozen_bn_act_bwd'](_ptr(dy), _ptr(y) if y is not None else None, _ptr(dx), _ptr(dres) if dres is not None else None,
                                          _dtype_code(dy), _ptr(scale), n_pix, c, _stream()), 'cms_frozen_bn_act_bwd')
        return dx, None, None, dres, None


def frozen_bn_act(x_nhwc, scale, shift, relu=False, res=None):
    """relu(x * scale + shift (+ res)): an eval-mode BatchNorm (+ residual, + ReLU) with a non-trainable affine on a contiguous NHWC
    bf16 / fp32 tensor (channels % 8 == 0); scale, shift fp32 [C]."""
    _need_cuda(x_nhwc, scale, shift, res)
    if not x_nhwc.is_contiguous() or x_nhwc.shape[-1] % 8 != 0 or x_nhwc.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError('frozen_bn_act: contiguous NHWC bf16 / fp32 tensor with channels % 8 == 0 required')
    if res is not None and (res.shape != x_nhwc.shape or res.dtype != x_nhwc.dtype or not res.is_contiguous()):
        raise ValueError('frozen_bn_act: residual must match the input')
    if scale.dtype != torch.float32 or shift.dtype != torch.float32 or scale.numel() != x_nhwc.shape[-1] or shift.numel() != x_nhwc.shape[-1]:
        raise ValueError('frozen_bn_act: fp32 scale / shift of one value per channel required')
    return _FrozenBnActFn.apply(x_nhwc, scale.contiguous(), shift.contiguous(), res, bool(relu))


def batch_norm_act(x_nhwc, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, relu=False, res=None,
                   group=None, groups=1):
    """nn.BatchNorm2d in training mode (+ residual add, + ReLU) on a contiguous NHWC tensor (channels %% 8 == 0).
    Updates the running statistics in place like the module does (once per sample group, in order)."""
    _need_cuda(x_nhwc, gamma, beta, running_mean, running_var, res)
    if not x_nhwc.is_contiguous() or x_nhwc.shape[-1] % 8 != 0 or x_nhwc.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError('batch_norm_act: contiguous NHWC bf16 / fp32 tensor with channels % 8 == 0 required')
    if res is not None and (res.shape != x_nhwc.shape or res.dtype != x_nhwc.dtype or not res.is_contiguous()):
        raise ValueError('batch_norm_act: residual must match the input')
    groups = int(groups)
    if groups < 1 or x_nhwc.shape[0] % groups != 0:
        raise ValueError('batch_norm_act: {} sample groups do not divide a batch of {}'.format(groups, x_nhwc.shape[0]))
    return _BatchNormActFn.apply(x_nhwc, gamma, beta, res, running_mean, running_var, momentum, eps, relu, group, groups)


def bn_workspace(n_pixels, c, device, groups=1):
    """Zero-filled workspace of one call site of the atomics-free BatchNorm reductions (cms_bn_workspace_bytes): tile counters
    + partial sums; the kernels leave it ready for their next launch, launches on different streams must not share it."""
    n = int(fn['cms_bn_workspace_bytes'](int(n_pixels), int(c), int(groups)))
    if n == 0:
        raise ValueError('bn_workspace: bad geometry ({} pixel rows, {} channels, {} groups)'.format(n_pixels, c, groups))
    ws = torch.empty((n + 3) // 4, dtype=torch.int32, device=device)
    counters = ((int(c) + 63) // 64 * 4 + 255) // 256 * 64      # int32 words: one counter per 64-channel tile, padded to 256 B
    ws[:min(ws.numel(), counters)].zero_()      # only the counters need a defined start; the partial sums are written first
    return ws


def bn_op(what, c=0, dtype=None, n_pixels=0, count=0.0, relu=False, eps=1e-5, momentum=0.1, groups=1, tile_rows=0, **t):
    """One launch of the batch-statistics BatchNorm protocol (csrc/bn.hip: cms_bn_run) on caller-owned buffers -- issued now, or
    appended to the program being recorded (cms_program_add_bn): the executor's batch-statistics passes (backbone_hip.py) are made
    of these. `what`: reduce | finalize | apply | reduce_bwd | bwd_apply | count | stats (= reduce + finalize in one launch) |
    finalize_tiles (statistics from the tile sums the unit's convolution wrote: ws = conv_igemm's stats['tile_sums'], tile_rows) |
    sums_tiles (backward sums from the tile sums of the data-gradient launch that wrote dy: ws, tile_rows -> sums);
    tensors by keyword (x, res, y, dy, dx, dres, sums, gamma, beta, mean, rstd, scale, shift, running_mean, running_var,
    counter, clear_a, clear_b, ws, mask_bits). `mask_bits` (uint8 [pixel rows][c / 8]): 'apply' writes [y > 0] there as bits,
    'reduce_bwd' (with ws) / 'bwd_apply' read them instead of y (1/16 of its bytes; bit-identical results). With `ws` (bn_workspace)
    the reductions take the atomics-free kernels; `groups` > 1 (sample groups normalised separately) needs them. `count` = pixels
    of one group. include/cutmixseg.h (cms_bn_op) says which kind reads which field."""
    _need_cuda(*t.values())
    if int(groups) > 1 and what in ('reduce', 'reduce_bwd') and t.get('ws') is None:
        raise ValueError('bn_op: grouped reductions need a workspace')
    d = _bn_desc(what, c, dtype, n_pixels, count, relu, eps, momentum, groups, tile_rows, **t)
    if _REC is None:
        _bn_run(d)
        return
    prog = _REC[0]
    idx = fn['cms_program_add_bn'](prog.h, C.byref(d), _rec_stream_index(), prog.group)
    if idx < 0:
        check(idx, 'cms_program_add_bn')
    prog.keep += [v for v in t.values() if v is not None]
    prog.bn_kinds[what] = prog.bn_kinds.get(what, 0) + 1


# ---------------------------------------------------------------------------------------------- stem
def stem_out_hw(h, w):
    """-> (ho, wo, hp, wp): sizes after the 7x7/2 convolution and after the ceil-mode 3x3/2 max-pool."""
    v = [C.c_int() for _ in range(4)]
    check(fn['cms_stem_out_hw'](int(h), int(w), *[C.byref(t) for t in v]), 'cms_stem_out_hw')
    return tuple(t.value for t in v)


def stem_pack_weights(w_packed_khkwcoci, out=None):
    """(49, 64, 3) fp32 / bf16 view of conv1.weight in the arena's physical layout -> fp32 (147 + 176, 64): rows
    0..146 = [c,ky,kx][co], the rest = the bf16 (hi, lo) MFMA fragments of the bf16 forward (csrc/stem.hip)."""
    _need_cuda(w_packed_khkwcoci, out)
    if tuple(w_packed_khkwcoci.shape) != (49, 64, 3) or not w_packed_khkwcoci.is_contiguous():
        raise ValueError('stem_pack_weights: contiguous (49, 64, 3) weight view required')
    if out is None:
        # 147 x 64 floats ([tap][co], the VALU kernels and the image gradient) + 2 x 64 x 22 x 8 bf16 behind them: the
        # (hi, lo) MFMA fragments of the bf16 forward = 176 more rows of 64 floats
        out = torch.empty((147 + 176, 64), dtype=torch.float32, device=w_packed_khkwcoci.device)
    if out.dtype != torch.float32 or out.numel() < (147 + 176) * 64 or not out.is_contiguous():
        raise ValueError('stem_pack_weights: `out` must be a contiguous fp32 buffer of at least (147 + 176) x 64 elements')
    check(fn['cms_stem_pack_weights'](_ptr(w_packed_khkwcoci), _dtype_code(w_packed_khkwcoci), _ptr(out), _stream()),
          'cms_stem_pack_weights')
    return out


def stem_forward(x, w147, scale, bias, out_dtype):
    """relu(bn(conv7x7/2(x))) -> (N, ho, wo, 64) NHWC; x (N, 3, H, W) NCHW-contiguous fp32 / bf16."""
    _need_cuda(x, w147, scale, bias)
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError('stem_forward: contiguous (N, 3, H, W) input required')
    n, _, h, w = (int(v) for v in x.shape)
    ho, wo, _, _ = stem_out_hw(h, w)
    y = torch.empty((n, ho, wo, 64), dtype=out_dtype, device=x.device)
    check(fn['cms_stem_fwd'](_ptr(x), _dtype_code(x), _ptr(y), _dtype_code(y), _ptr(w147), _ptr(scale), _ptr(bias), n, h, w,
                             _stream()), 'cms_stem_fwd')
    return y


def _pool_out(v, ceil_mode):
    if not ceil_mode:
        return (v + 2 - 3) // 2 + 1
    r = (v + 2 - 3 + 1) // 2 + 1            # ATen's ceil-mode output size for kernel 3, stride 2, padding 1
    return r - 1 if (r - 1) * 2 >= v + 1 else r


def maxpool3x3s2_forward(s, ceil_mode=True, out=None):
    """3x3 / 2 / pad 1 max-pool of an NHWC tensor -> (pooled, argmax uint8). `out`: the pooled tensor's buffer (the persistent
    input buffer of a recorded body pass: backbone_hip._StemFn), else a new tensor."""
    _need_cuda(s, out)
    n, hs, ws, c = (int(v) for v in s.shape)
    hp, wp = _pool_out(hs, ceil_mode), _pool_out(ws, ceil_mode)
    if out is not None:
        if tuple(out.shape) != (n, hp, wp, c) or out.dtype != s.dtype or not out.is_contiguous():
            raise ValueError('maxpool3x3s2_forward: `out` must be a contiguous {} tensor of shape {}'.format(s.dtype, (n, hp, wp, c)))
        p = out
    else:
        p = torch.empty((n, hp, wp, c), dtype=s.dtype, device=s.device)
    idx = torch.empty((n, hp, wp, c), dtype=torch.uint8, device=s.device)
    check(fn['cms_maxpool3x3s2_fwd'](_ptr(s), _ptr(p), _ptr(idx), _dtype_code(s), n, hs, ws, c, int(bool(ceil_mode)),
                                     _stream()), 'cms_maxpool3x3s2_fwd')
    return p, idx


def maxpool3x3s2_relu_backward(dp, idx, s, ceil_mode=True):
    """gradient wrt the PRE-ReLU stem output: [s > 0] * max-pool backward."""
    _need_cuda(dp, idx, s)
    dp = dp.contiguous()
    if dp.dtype != s.dtype or dp.shape != idx.shape:
        raise ValueError('maxpool backward: dtype / shape mismatch')
    n, hs, ws, c = (int(v) for v in s.shape)
    ds = torch.empty_like(s)
    check(fn['cms_maxpool3x3s2_relu_bwd'](_ptr(dp), _ptr(idx), _ptr(s), _ptr(ds), _dtype_code(s), n, hs, ws, c,
                                          int(bool(ceil_mode)), _stream()), 'cms_maxpool3x3s2_relu_bwd')
    return ds


def stem_wgrad(x, ds, dw_khkwcoci, scale):
    """dw (49, 64, 3) fp32 view of conv1.weight's gradient in the arena, accumulated into."""
    _need_cuda(x, ds, dw_khkwcoci, scale)
    if tuple(dw_khkwcoci.shape) != (49, 64, 3) or dw_khkwcoci.dtype != torch.float32 or not dw_khkwcoci.is_contiguous():
        raise ValueError('stem_wgrad: contiguous fp32 (49, 64, 3) gradient view required')
    n, _, h, w = (int(v) for v in x.shape)
    ws, nbytes = None, 0
    if deterministic_wgrad():
        nbytes = int(fn['cms_stem_wgrad_workspace_bytes'](_dtype_code(x), _dtype_code(ds), n, h, w))
        key = ('stem', x.device.index, int(torch.cuda.current_stream().cuda_stream))
        ws = _WGRAD_WS.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _WGRAD_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(fn['cms_stem_wgrad_ws'](_ptr(x), _dtype_code(x), _ptr(ds), _dtype_code(ds), _ptr(dw_khkwcoci), _ptr(scale), n, h, w,
                                  _ptr(ws), nbytes, _stream()), 'cms_stem_wgrad_ws')


def stem_dgrad(ds, w147, scale, x_shape):
    _need_cuda(ds, w147, scale)
    n, _, h, w = (int(v) for v in x_shape)
    dx = torch.empty((n, 3, h, w), dtype=torch.float32, device=ds.device)
    check(fn['cms_stem_dgrad'](_ptr(ds), _dtype_code(ds), _ptr(w147), _ptr(scale), _ptr(dx), n, h, w, _stream()),
          'cms_stem_dgrad')
    return dx


def bn_fold(flat, idx_weight, idx_bias, idx_mean, idx_var, eps, scale, bias):
    """scale = flat[idx_weight] * rsqrt(flat[idx_var] + eps); bias = flat[idx_bias] - flat[idx_mean] * scale -- frozen BatchNorm of
    all layers folded in one launch (csrc/optim.hip: cms_bn_fold; deeplab2.py:92-107)."""
    _need_cuda(flat, idx_weight, idx_bias, idx_mean, idx_var, scale, bias)
    n = int(scale.numel())
    if flat.dtype != torch.float32 or scale.dtype != torch.float32 or bias.dtype != torch.float32 \
            or any(t.dtype != torch.int64 or int(t.numel()) != n or not t.is_contiguous() for t in (idx_weight, idx_bias, idx_mean, idx_var)) \
            or int(bias.numel()) != n or not (scale.is_contiguous() and bias.is_contiguous() and flat.is_contiguous()):
        raise TypeError('bn_fold: fp32 arena / outputs and int64 index tables of the outputs\' length required')
    check(fn['cms_bn_fold'](_ptr(flat), _ptr(idx_weight), _ptr(idx_bias), _ptr(idx_mean), _ptr(idx_var), n, float(eps), _ptr(scale),
                            _ptr(bias), _stream()), 'cms_bn_fold')


# ---------------------------------------------------------------------------------------------- launch programs
HBM_PEAK_BPS, MFMA_PEAK_FLOPS = 8.0e12, 2.5e15       # MI355X_MICROARCH.md: HBM3E, dense bf16 MFMA


class Program(object):
    """A recorded network pass (csrc/program.hip): launch descriptors over persistent buffers, replayed from C++ with
    one call. Record with `with recording(prog, [main_stream, side_stream, ...]):` around ordinary calls of
    conv_igemm / conv_wgrad / memset_zero / stream_wait -- inside the block they append to the program instead of
    launching. Stream indices are positions in the list given to `recording` / `run`."""

    def __init__(self):
        h = C.c_void_p()
        check(fn['cms_program_create'](C.byref(h)), 'cms_program_create')
        self.h = h
        self.keep = []          # every tensor a descriptor points into stays alive as long as the program
        self.marks = []         # (op index, tag): segment boundaries for callers that interleave host work
        self.group = 0          # interleaving key given to the ops recorded next (run_pair)
        self.flops = 0.0        # algorithmic MFMA FLOPs of one replay (convolutions + weight gradients)
        self.conv_launches = 0
        self.conv_bytes = 0.0   # algorithmic HBM bytes of the convolution launches (operands once, output once)
        self.head_bytes = 0.0   # bytes the ASPP head launches MOVE (incl. the fp32 Z planes the GEMM writes and the gather re-reads)
        self.head_bytes_alg = 0.0   # ... their ALGORITHMIC bytes per SURVEY 8(d): the 2048-channel input once + weights + logits
        self.floor_s = 0.0      # sum over the convolution / weight-gradient launches of max(bytes / 8 TB/s, FLOPs / 2.5 PFLOP/s):
                                # the mixed HBM / MFMA roofline of one replay (bench.py: roofline.mixed)
        self.head_launches = 0
        self.by_route = {}      # kernel route (cms_conv_igemm_route / 'wgrad8' / 'wgrad128') -> [launches, algorithmic bytes, FLOPs]
        self.n_streams = 1
        self.bn_kinds = {}      # BatchNorm launches recorded, by kind ('stats', 'finalize_tiles', 'sums_tiles', 'reduce', ...)
        self.host_ops = []      # (op index, stream index, callable): host work between two launches of a replay -- the
                                # all-reduces of SyncBN statistics (recorded with `host_call`); `run` splits around them

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h is not None:
            try:
                fn['cms_program_destroy'](h)
            except Exception:
                pass

    def size(self):
        return int(fn['cms_program_size'](self.h))

    def mark(self, tag):
        self.marks.append((self.size(), tag))

    @staticmethod
    def _handles(streams):
        arr = (C.c_void_p * len(streams))()
        for i, st in enumerate(streams):
            arr[i] = st.cuda_stream
        return arr

    def run(self, streams, first=0, last=-1):
        if len(streams) < self.n_streams:
            raise ValueError('program recorded on {} streams, {} given'.format(self.n_streams, len(streams)))
        if self.host_ops:
            # a host op recorded at index i happens after launches [0, i) and before launch i: it belongs to the range that
            # STARTS at i (segmented replays call run(first, i) and then run(i, ...)), or to the last range when i == size
            size = self.size()
            end = size if (last < 0 or last >= size) else int(last)
            handles = self._handles(streams)
            pos = int(first)
            for idx, si, call in self.host_ops:          # recorded in program order
                if idx < pos or idx > end or (idx == end and end != size):
                    continue
                if idx > pos:
                    check(fn['cms_program_run'](self.h, pos, idx, handles, len(streams)), 'cms_program_run')
                    pos = idx
                with torch.cuda.stream(streams[si]):
                    call()
            if pos < end:
                check(fn['cms_program_run'](self.h, pos, end, handles, len(streams)), 'cms_program_run')
            return
        check(fn['cms_program_run'](self.h, int(first), int(last), self._handles(streams), len(streams)),
              'cms_program_run')

    def set_timing(self, every_k):
        check(fn['cms_program_set_timing'](self.h, int(every_k)), 'cms_program_set_timing')

    def read_timing(self):
        """-> dict(ms, flops, launches, head_ms, head_launches) of the event-bracketed convolution launches since the
        last call (waits for them)."""
        ms, fl, n = C.c_double(), C.c_double(), C.c_long()
        hms, hn = C.c_double(), C.c_long()
        check(fn['cms_program_read_timing'](self.h, C.byref(ms), C.byref(fl), C.byref(n), C.byref(hms), C.byref(hn)),
              'cms_program_read_timing')
        return dict(ms=ms.value, flops=fl.value, launches=n.value, head_ms=hms.value, head_launches=hn.value)


def run_pair(prog_a, streams_a, prog_b, streams_b):
    """Two programs issued interleaved group by group (student on one stream, teacher on another). Programs with host
    operations between their launches (SyncBN all-reduces) cannot be interleaved from the native side: refused, so that a
    caller can never drop the exchanges silently (`_BodyPairFn` issues such passes one after the other)."""
    if prog_a.host_ops or prog_b.host_ops:
        raise RuntimeError('run_pair: a program with host operations (SyncBN exchanges) must be replayed with Program.run')
    check(fn['cms_program_run_pair'](prog_a.h, Program._handles(streams_a), len(streams_a), prog_b.h,
                                     Program._handles(streams_b), len(streams_b)), 'cms_program_run_pair')


_REC = None      # (Program, [cuda_stream handles]) while recording


class recording(object):
    def __init__(self, prog, streams):
        self.prog, self.streams = prog, [st.cuda_stream for st in streams]
        prog.n_streams = max(prog.n_streams, len(streams))

    def __enter__(self):
        global _REC
        if _REC is not None:
            raise RuntimeError('nested program recording')
        _REC = (self.prog, self.streams)
        return self.prog

    def __exit__(self, *exc):
        global _REC
        _REC = None


def _rec_stream_index(stream=None):
    h = (torch.cuda.current_stream() if stream is None else stream).cuda_stream
    try:
        return _REC[1].index(h)
    except ValueError:
        raise RuntimeError('op recorded on a stream the program was not told about')


def host_call(call):
    """Host work at this point of the current stream: run now, or -- while recording -- at this point of every replay (between
    two native launch calls: Program.run splits around it). Used for the all-reduce of SyncBN statistics, which is issued by
    torch.distributed and cannot be a launch descriptor."""
    if _REC is None:
        call()
        return
    prog = _REC[0]
    prog.host_ops.append((prog.size(), _rec_stream_index(), call))


def memset_zero(t):
    """t.zero_() -- as a program op while recording."""
    _need_cuda(t)
    if _REC is None:
        t.zero_()
        return t
    if not t.is_contiguous():
        raise TypeError('memset_zero: contiguous tensor required')
    prog = _REC[0]
    idx = fn['cms_program_add_memset'](prog.h, _ptr(t), t.numel() * t.element_size(), _rec_stream_index(), prog.group)
    if idx < 0:
        check(idx, 'cms_program_add_memset')
    prog.keep.append(t)
    return t


def stream_wait(waiter, waited):
    """waiter.wait_stream(waited) -- as a program op while recording."""
    if _REC is None:
        waiter.wait_stream(waited)
        return
    prog = _REC[0]
    idx = fn['cms_program_add_sync'](prog.h, _rec_stream_index(waited), _rec_stream_index(waiter), prog.group)
    if idx < 0:
        check(idx, 'cms_program_add_sync')


# ---------------------------------------------------------------------------------------------- ASPP head
def _tap_arrays(taps):
    n = len(taps)
    dy = (C.c_int * n)(*[int(t[0]) for t in taps])
    dx = (C.c_int * n)(*[int(t[1]) for t in taps])
    return dy, dx, n


def aspp_gather_fwd(z, bias, taps, num_classes, out=None):
    """logits[n][c][y][x] = bias[c] + sum_t z[n][t*C + c][y + dy_t][x + dx_t]; z fp32 (N, ZC, h, w) (csrc/aspp.hip)."""
    _need_cuda(z, bias, out)
    if z.dtype != torch.float32 or not z.is_contiguous():
        raise TypeError('aspp_gather_fwd: contiguous fp32 (N, ZC, h, w) input required')
    n, zc, h, w = (int(v) for v in z.shape)
    if out is None:
        out = torch.empty((n, int(num_classes), h, w), dtype=torch.float32, device=z.device)
    dy, dx, nt = _tap_arrays(taps)
    if _REC is not None:
        prog = _REC[0]
        idx = fn['cms_program_add_aspp_gather'](prog.h, _ptr(z), _ptr(bias), _ptr(out), dy, dx, nt, n, int(num_classes), zc,
                                                h, w, _rec_stream_index(), prog.group)
        if idx < 0:
            check(idx, 'cms_program_add_aspp_gather')
        prog.keep += [t for t in (z, bias, out) if t is not None]
        prog.head_bytes += 4.0 * nt * int(num_classes) * n * h * w + 4.0 * out.numel()
        prog.head_bytes_alg += 4.0 * out.numel()
        return out
    check(fn['cms_aspp_gather_fwd'](_ptr(z), _ptr(bias), _ptr(out), dy, dx, nt, n, int(num_classes), zc, h, w, _stream()),
          'cms_aspp_gather_fwd')
    return out


def aspp_spread_bwd(dlogits, taps, zc, dtype, out=None):
    """D[n][y][x][t*C + c] = dlogits[n][c][y - dy_t][x - dx_t] -> NHWC (N, h, w, zc) operand of the head's backward GEMMs."""
    _need_cuda(dlogits, out)
    if dlogits.dtype != torch.float32 or not dlogits.is_contiguous():
        raise TypeError('aspp_spread_bwd: contiguous fp32 (N, C, h, w) gradient required')
    n, c, h, w = (int(v) for v in dlogits.shape)
    if out is None:
        out = torch.empty((n, h, w, int(zc)), dtype=dtype, device=dlogits.device)
    dy, dx, nt = _tap_arrays(taps)
    if _REC is not None:
        prog = _REC[0]
        idx = fn['cms_program_add_aspp_spread'](prog.h, _ptr(dlogits), _ptr(out), _dtype_code(out), dy, dx, nt, n, c,
                                                int(zc), h, w, _rec_stream_index(), prog.group)
        if idx < 0:
            check(idx, 'cms_program_add_aspp_spread')
        prog.keep += [dlogits, out]
        return out
    check(fn['cms_aspp_spread_bwd'](_ptr(dlogits), _ptr(out), _dtype_code(out), dy, dx, nt, n, c, int(zc), h, w, _stream()),
          'cms_aspp_spread_bwd')
    return out


# ---------------------------------------------------------------------------------------------- MFMA convolution
_ZERO_PAGES = {}


def _zero_page(device):
    """An all-zero device buffer: where the direct-to-LDS loader fetches padded / out-of-range rows from (it walks
    through it like through a pixel's channel run, so it must be >= 2 * Cin + 128 bytes: 64 KB covers Cin <= 32704)."""
    z = _ZERO_PAGES.get(device)
    if z is None:
        z = torch.zeros(32768, dtype=torch.bfloat16, device=device)
        _ZERO_PAGES[device] = z
    return z


# cms_conv_igemm_route -> the kernel name rocprofv3 reports (prefix)
_ROUTE_NAMES = {8: 'conv8_kernel', 2: 'conv_igemm_mixed_kernel', 1: 'conv_igemm_kernel<2, 2, 2, 2', 3: 'conv_igemm_kernel<1, 4, 2, 1',
                4: 'conv_igemm_kernel<1, 4, 1, 1', 0: 'other'}


def conv_taps(kh, kw, dilation, padding):
    """(dy, dx) input offsets of the kh*kw taps in [ky][kx] order."""
    return [(ky * dilation - padding, kx * dilation - padding) for ky in range(kh) for kx in range(kw)]


def conv_igemm(x, w_packed, taps, stride=1, out_hw=None, scale=None, bias=None, res=None, relu=False, mode=0,
               mask_src=None, out=None, out_f32_nchw=None, cout_real=None, out_stride=1, out_full_hw=None, tile=0,
               ksplit=1, variant=0, out_pixel_offset=0, mask_bits_out=None, mask_bits=None, stats=None,
               mask_gates_res=False):
    """
    Implicit-GEMM convolution on the MFMA units (csrc/conv.hip).
      x         bf16 NHWC-contiguous tensor of logical shape (N, H, W, Cin)
      w_packed  bf16 (ntaps, Cout, Cin)
      taps      list of (dy, dx) input offsets per tap
    Returns the bf16 (N, out_h, out_w, Cout) output (or the fp32 NCHW tensor given in `out_f32_nchw`).
    `out_pixel_offset` (with `out`, `out_stride` > 1): the strided scatter starts at that pixel of the output tensor
    instead of pixel 0 -- residual / mask are read at the same shifted positions (the phases of a transposed convolution).
    `mask_bits_out` (forward + ReLU): uint8 (N, out_h, out_w, Cout / 8) that receives [y > 0] as bits; `mask_bits` (mode 1):
    such a tensor INSTEAD of `mask_src` -- the ReLU mask of a data gradient at 1/16 of the bytes (cms_conv_desc).
    `mask_gates_res` (mode 1 with `res` and `mask_bits`): the bits gate the residual only, y = acc + (bit ? res : 0).
    `stats` (bf16 forward launches): a dict {'groups': G}; when the kernel that takes the launch can, its epilogue also writes the
    per-channel (sum, sum of squares) of every pixel tile it stores (cms_conv_desc.stats_out) and the dict comes back with
    'tile_rows' (128 / 256) and 'tile_sums' (fp32 [tiles][2][2][Cout]) for bn_op('finalize_tiles'); 'tile_rows' = 0 when it cannot
    (the statistics then take a pass over the output: bn_op('stats')). Data gradients (mode 1): the dict also carries 'u', 'mean',
    'rstd' and optionally 'bits' of the batch-statistics unit whose OUTPUT gradient the launch writes; the tile sums are then
    (sum d, sum d * xhat) for bn_op('sums_tiles') (cms_conv_desc.bstats_*).
    """
    _need_cuda(x, w_packed, scale, bias, res, mask_src, out, out_f32_nchw, mask_bits_out, mask_bits)
    for t in (mask_bits_out, mask_bits):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or x.dtype != torch.bfloat16):
            raise TypeError('conv_igemm: ReLU mask bits are contiguous uint8 tensors of the bf16 entry point')
    if mask_bits is not None and mask_src is not None:
        raise ValueError('conv_igemm: mask_bits replaces mask_src')
    if mask_gates_res and (mask_bits is None or res is None or int(mode) != 1):
        raise ValueError('conv_igemm: mask_gates_res needs a data-gradient launch with res and mask_bits')
    if x.dtype not in (torch.bfloat16, torch.float32) or w_packed.dtype != x.dtype or not x.is_contiguous() \
            or not w_packed.is_contiguous():
        raise TypeError('conv_igemm: contiguous NHWC input and packed weights of one dtype (bf16 or fp32) required')
    for t in (res, mask_src, out):
        if t is not None and (t.dtype != x.dtype or not t.is_contiguous()):
            raise TypeError('conv_igemm: residual / mask / output tensors must be contiguous and of the input dtype')
    f32 = x.dtype == torch.float32          # fp32 parity configuration: csrc/conv_f32.hip
    n, h, w_in, cin = (int(s) for s in x.shape)
    ntaps, cout, cin_w = (int(s) for s in w_packed.shape)
    if cin_w != cin or ntaps != len(taps):
        raise ValueError('conv_igemm: weight / tap table does not match the input')
    ho, wo = (int(out_hw[0]), int(out_hw[1])) if out_hw is not None else (h, w_in)
    oh, ow = (int(out_full_hw[0]), int(out_full_hw[1])) if out_full_hw is not None else (ho, wo)
    d = _lib.ConvDesc()
    d.x, d.w = x.data_ptr(), w_packed.data_ptr()
    if out_f32_nchw is None:
        if out is None:
            out = torch.empty((n, oh, ow, cout), dtype=x.dtype, device=x.device)
            if out_stride > 1:
                memset_zero(out)               # the strided scatter only visits every out_stride-th position
        shift = int(out_pixel_offset) * cout * x.element_size()
        if shift and (out_stride <= 1 or out is None):
            raise ValueError('conv_igemm: out_pixel_offset needs a caller-owned `out` and out_stride > 1')
        d.y, d.y32 = out.data_ptr() + shift, None
    else:
        d.y, d.y32 = None, out_f32_nchw.data_ptr()
    d.scale = scale.data_ptr() if scale is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    shift = int(out_pixel_offset) * cout * x.element_size() if out_f32_nchw is None else 0
    d.res = res.data_ptr() + shift if res is not None else None
    d.mask_src = mask_src.data_ptr() + shift if mask_src is not None else None
    d.n, d.h, d.w_in, d.cin = n, h, w_in, cin
    bshift = int(out_pixel_offset) * (int(w_packed.shape[1]) // 8) if out_f32_nchw is None else 0
    d.mask_bits_out = mask_bits_out.data_ptr() + bshift if mask_bits_out is not None else None
    d.mask_bits = mask_bits.data_ptr() + bshift if mask_bits is not None else None
    d.mask_gates_res = int(bool(mask_gates_res))
    d.ho, d.wo, d.cout = ho, wo, cout
    d.cout_real = cout if cout_real is None else int(cout_real)
    d.ntaps = ntaps
    for i, (dy, dx) in enumerate(taps):
        d.tap_dy[i], d.tap_dx[i] = int(dy), int(dx)
    d.stride = int(stride)
    d.out_h, d.out_w, d.out_stride = oh, ow, int(out_stride)
    d.relu, d.mode, d.tile = int(bool(relu)), int(mode), int(tile)
    d.ksplit = int(ksplit)
    zp = _zero_page(x.device)
    d.zeros, d.zeros_bytes = zp.data_ptr(), zp.numel() * 2
    d.variant = int(variant)
    tile_sums = None
    if stats is not None:
        stats['tile_rows'], stats['tile_sums'] = 0, None
        G = max(1, int(stats.get('groups', 1)))
        M = n * ho * wo
        if not f32 and out_f32_nchw is None and M % G == 0:
            d.stats_rows_per_group = M // G
            if stats.get('u') is not None:          # backward statistics of the unit whose output gradient this launch writes
                u_, mean_, rstd_, bits_ = stats['u'], stats['mean'], stats['rstd'], stats.get('bits')
                _need_cuda(u_, mean_, rstd_, bits_)
                if u_.dtype != x.dtype or not u_.is_contiguous() or u_.numel() != M * cout or mean_.numel() != G * cout \
                        or rstd_.numel() != G * cout or (bits_ is not None and (bits_.dtype != torch.uint8 or bits_.numel() * 8 != M * cout)):
                    raise ValueError('conv_igemm: backward statistics need u like the output, mean / rstd [groups][Cout], bits [pixels][Cout / 8]')
                d.bstats_u, d.bstats_mean, d.bstats_rstd = u_.data_ptr(), mean_.data_ptr(), rstd_.data_ptr()
                d.bstats_bits = bits_.data_ptr() if bits_ is not None else None
            rows = int(fn['cms_conv_igemm_stats_tile_rows'](C.byref(d)))
            if rows < 0:
                check(rows, 'cms_conv_igemm_stats_tile_rows')
            if rows > 0:
                tile_sums = torch.empty(((M + rows - 1) // rows) * 4 * cout, dtype=torch.float32, device=x.device)
                d.stats_out = tile_sums.data_ptr()
                stats['tile_rows'], stats['tile_sums'] = rows, tile_sums
    if _REC is not None:
        prog = _REC[0]
        idx = fn['cms_program_add_conv'](prog.h, C.byref(d), int(f32), _rec_stream_index(), prog.group)
        if idx < 0:
            check(idx, 'cms_program_add_conv')
        prog.keep += [t for t in (x, w_packed, out, out_f32_nchw, scale, bias, res, mask_src, zp, mask_bits_out, mask_bits, tile_sums)
                      if t is not None]
        if stats is not None:
            prog.keep += [t for t in (stats.get('u'), stats.get('mean'), stats.get('rstd'), stats.get('bits')) if t is not None]
        esz = x.element_size()
        prog.flops += 2.0 * n * ho * wo * cout * cin * ntaps
        nbytes = esz * (x.numel() + w_packed.numel()) + float(n * ho * wo) * (
            (4.0 * d.cout_real if out_f32_nchw is not None else esz * cout)
            + (esz * cout if res is not None else 0.0) + (esz * cout if mask_src is not None else 0.0)
            + (cout / 8.0 if mask_bits is not None else 0.0) + (cout / 8.0 if mask_bits_out is not None else 0.0)
            + ((esz * cout + (cout / 8.0 if stats.get('bits') is not None else 0.0))
               if (stats is not None and stats.get('u') is not None and stats.get('tile_rows')) else 0.0))
        # (the head's fp32 Z planes are an intermediate of the single-pass formulation, not algorithmic output: its floor counts
        # the input and the weights here and the logits at the gather)
        fbytes = esz * (x.numel() + w_packed.numel()) if (out_f32_nchw is not None and d.cout_real > 32) else nbytes
        prog.floor_s += max(fbytes / HBM_PEAK_BPS, 2.0 * n * ho * wo * cout * cin * ntaps / MFMA_PEAK_FLOPS)
        if not f32:
            route = _ROUTE_NAMES.get(int(fn['cms_conv_igemm_route'](C.byref(d))), 'other')
            r = prog.by_route.setdefault(route, [0, 0.0, 0.0])
            r[0] += 1; r[1] += nbytes; r[2] += 2.0 * n * ho * wo * cout * cin * ntaps
        if out_f32_nchw is not None:
            prog.head_launches += 1
            prog.head_bytes += nbytes
            prog.head_bytes_alg += esz * (x.numel() + w_packed.numel())      # (its Z planes are an intermediate, not an output)
        else:
            prog.conv_launches += 1
            prog.conv_bytes += nbytes
        return out if out_f32_nchw is None else out_f32_nchw
    name = 'cms_conv_igemm_f32' if f32 else 'cms_conv_igemm'
    check(fn[name](C.byref(d), _stream()), name)
    return out if out_f32_nchw is None else out_f32_nchw


def conv_pack_transpose(w_packed, scale=None, flip=True, out=None, out_dtype=None):
    """(ntaps, Cout, Cin) fp32/bf16 -> bf16 (ntaps, Cin, Cout) with BN scale folded and taps flipped: dgrad operand.
    `out_dtype=torch.float32` (fp32 source only) gives the operand of the fp32 parity configuration."""
    _need_cuda(w_packed, scale, out)
    ntaps, cout, cin = (int(s) for s in w_packed.shape)
    if not w_packed.is_contiguous():
        raise TypeError('conv_pack_transpose: contiguous weights required')
    if out_dtype == torch.float32 or (out is not None and out.dtype == torch.float32):
        if w_packed.dtype != torch.float32:
            raise TypeError('conv_pack_transpose: an fp32 destination needs an fp32 source')
        if out is None:
            out = torch.empty((ntaps, cin, cout), dtype=torch.float32, device=w_packed.device)
        check(fn['cms_conv_pack_transpose_f32'](_ptr(w_packed), _ptr(out), _ptr(scale), ntaps, cout, cin,
                                                int(bool(flip)), _stream()), 'cms_conv_pack_transpose_f32')
        return out
    if out is None:
        out = torch.empty((ntaps, cin, cout), dtype=torch.bfloat16, device=w_packed.device)
    check(fn['cms_conv_pack_transpose'](_ptr(w_packed), _dtype_code(w_packed), _ptr(out), _ptr(scale), ntaps, cout, cin,
                                        int(bool(flip)), _stream()), 'cms_conv_pack_transpose')
    return out


class PackTransposePlan(object):
    """Device-resident item table for cms_conv_pack_transpose_batch: (src (ntaps,Cout,Cin), dst, scale) triples with
    fixed addresses, re-packed in ONE launch (`run()`)."""

    def __init__(self, triples):
        items = (_lib.PackItem * len(triples))()
        blk = 0
        self._keep = triples
        dt = triples[0][0].dtype
        ddt = triples[0][1].dtype
        if ddt not in (torch.bfloat16, torch.float32) or (ddt == torch.float32 and dt != torch.float32):
            raise TypeError('PackTransposePlan: bf16 destinations, or fp32 destinations from fp32 sources')
        self.dst_f32 = ddt == torch.float32
        # (round 6) 64 x 64 tiles with 16-byte accesses where every tensor allows it (bf16 -> bf16, channel counts % 64 == 0: the
        # DeepLab bodies); CMS_PACK64=0 keeps the 32 x 32 kernel (A/B)
        self.tile64 = (dt == torch.bfloat16 and ddt == torch.bfloat16 and _os.environ.get('CMS_PACK64', '1') != '0'
                       and all(int(s.shape[1]) % 64 == 0 and int(s.shape[2]) % 64 == 0 for s, _, _ in triples))
        tl = 64 if self.tile64 else 32
        for i, (src, dst, scale) in enumerate(triples):
            _need_cuda(src, dst, scale)
            ntaps, cout, cin = (int(v) for v in src.shape)
            if src.dtype != dt or not src.is_contiguous() or not dst.is_contiguous() \
                    or tuple(dst.shape) != (ntaps, cin, cout) or dst.dtype != ddt:
                raise TypeError('PackTransposePlan: contiguous (ntaps,Cout,Cin) sources of one dtype, '
                                '(ntaps,Cin,Cout) destinations of one dtype')
            items[i].src, items[i].dst = src.data_ptr(), dst.data_ptr()
            items[i].scale = scale.data_ptr() if scale is not None else None
            items[i].ntaps, items[i].cout, items[i].cin, items[i].first_block = ntaps, cout, cin, blk
            blk += ntaps * ((cout + tl - 1) // tl) * ((cin + tl - 1) // tl)
        self.n_items, self.total_blocks = len(triples), blk
        self.dtype_code = _dtype_code(triples[0][0])
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(triples[0][0].device)

    def run(self):
        if self.dst_f32:
            check(fn['cms_conv_pack_transpose_batch_f32'](_ptr(self.table), self.n_items, self.total_blocks, _stream()),
                  'cms_conv_pack_transpose_batch_f32')
            return
        if self.tile64:
            check(fn['cms_conv_pack_transpose_batch64'](_ptr(self.table), self.n_items, self.total_blocks, _stream()),
                  'cms_conv_pack_transpose_batch64')
            return
        check(fn['cms_conv_pack_transpose_batch'](_ptr(self.table), self.n_items, self.total_blocks, self.dtype_code,
                                                  _stream()), 'cms_conv_pack_transpose_batch')


# Deterministic weight gradients (csrc/conv.hip: split-K partial sums through slabs + an ordered reduce instead of fp32
# atomics). Off by default: inside the two-stream step the atomics are 1.5-2 % faster (profiles/r03a_*). Switch on with
# `set_deterministic_wgrad(True)` (StepConfig.deterministic, the trainers' --deterministic) or CMS_WGRAD_SLAB=1.
import os as _os
_WGRAD_DETERMINISTIC = _os.environ.get('CMS_WGRAD_SLAB', '0') not in ('', '0', '2')
# CMS_WGRAD_SLAB=2 (experiment): slabs only for the large layers (|dW| >= 256 k elements: layer3 / layer4), atomics for the rest
_WGRAD_SLAB_LARGE = _os.environ.get('CMS_WGRAD_SLAB', '0') == '2'
_WGRAD_WS = {}            # (device index, stream handle) -> uint8 scratch of eagerly issued launches
if _WGRAD_DETERMINISTIC:
    fn['cms_loss_set_deterministic'](1)


def set_deterministic_wgrad(on):
    """Run-to-run deterministic weight gradients for every launch issued (or RECORDED) from now on."""
    global _WGRAD_DETERMINISTIC
    _WGRAD_DETERMINISTIC = bool(on)
    fn['cms_loss_set_deterministic'](int(bool(on)))     # the loss kernels' backward: colour classes instead of one launch


def deterministic_wgrad():
    return _WGRAD_DETERMINISTIC


def _wgrad_workspace(d, device, recording):
    """Scratch of exactly the size this launch needs (cms_conv_wgrad_workspace_bytes). A recorded launch owns its slab
    (kept alive by the program; replays on any stream never share it); eager launches reuse one buffer per stream
    (launches on one stream are serialised), grown on demand."""
    need = int(fn['cms_conv_wgrad_workspace_bytes'](C.byref(d)))
    if need <= 0:
        return None
    if recording:
        return torch.empty(need, dtype=torch.uint8, device=device)
    key = (device.index, int(torch.cuda.current_stream().cuda_stream))
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _WGRAD_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def conv_wgrad(du, x, taps, dw, stride=1, scale=None, cout_real=None, ksplit=0, w_bf16=None, wdot=None, dbeta=None,
               dw_cout=None, query_kernel=False, wg_target=0):
    """
    dw (fp32 (ntaps, Cout, Cin), accumulated into) += scale[co] * sum_pixels du[pix][co] * x[pix + tap][ci].
    du bf16 (N, Ho, Wo, Cout), x bf16 (N, H, W, Cin), both NHWC-contiguous. `dw_cout`: rows per tap of `dw` when it is
    narrower than du's (padded) channel axis -- only the first `cout_real` rows are written.
    `wg_target`: CUs the eight-phase kernel should aim at when the launch runs BESIDE other work (0 = it has the machine).
    `query_kernel`: launch nothing, return 8 if this call would take the eight-phase 256 x 256 kernel (csrc/wgrad8.hip), else 0.
    """
    _need_cuda(du, x, dw, scale)
    if du.dtype not in (torch.bfloat16, torch.float32) or x.dtype != du.dtype or dw.dtype != torch.float32:
        raise TypeError('conv_wgrad: bf16 (or fp32, parity configuration) activations of one dtype and an fp32 '
                        'gradient buffer required')
    f32 = du.dtype == torch.float32
    if not (du.is_contiguous() and x.is_contiguous() and dw.is_contiguous()):
        raise TypeError('conv_wgrad: contiguous tensors required')
    n, ho, wo, cout = (int(s) for s in du.shape)
    n2, h, w_in, cin = (int(s) for s in x.shape)
    if n2 != n or tuple(dw.shape) != (len(taps), cout if dw_cout is None else int(dw_cout), cin):
        raise ValueError('conv_wgrad: shape mismatch')
    if dw_cout is not None and (cout_real is None or int(cout_real) > int(dw_cout)):
        raise ValueError('conv_wgrad: dw_cout needs cout_real <= dw_cout')
    d = _lib.WgradDesc()
    d.du, d.x, d.dw = du.data_ptr(), x.data_ptr(), dw.data_ptr()
    d.scale = scale.data_ptr() if scale is not None else None
    d.n, d.h, d.w_in, d.cin, d.ho, d.wo, d.cout = n, h, w_in, cin, ho, wo, cout
    d.cout_real = 0 if cout_real is None else int(cout_real)
    d.ntaps = len(taps)
    for i, (dy, dx) in enumerate(taps):
        d.tap_dy[i], d.tap_dx[i] = int(dy), int(dx)
    d.stride = int(stride)
    d.ksplit = int(ksplit)
    # side outputs for a trainable BatchNorm affine behind this convolution (see cms_wgrad_desc)
    _need_cuda(w_bf16, wdot, dbeta)
    d.w = w_bf16.data_ptr() if w_bf16 is not None else None
    d.wdot = wdot.data_ptr() if wdot is not None else None
    d.dbeta = dbeta.data_ptr() if dbeta is not None else None
    d.dw_cout = 0 if dw_cout is None else int(dw_cout)
    d.wg_target = int(wg_target)
    if query_kernel:
        return 8 if (not f32 and int(fn['cms_conv_wgrad_uses_wgrad8'](C.byref(d)))) else 0
    ws = None
    if not f32 and (_WGRAD_DETERMINISTIC or (_WGRAD_SLAB_LARGE and len(taps) * cout * cin >= 262144)):
        ws = _wgrad_workspace(d, du.device, _REC is not None)
        if ws is not None:
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if _REC is not None:
        prog = _REC[0]
        idx = fn['cms_program_add_wgrad'](prog.h, C.byref(d), int(f32), _rec_stream_index(), prog.group)
        if idx < 0:
            check(idx, 'cms_program_add_wgrad')
        prog.keep += [t for t in (du, x, dw, scale, w_bf16, wdot, dbeta, ws) if t is not None]
        prog.flops += 2.0 * n * ho * wo * cout * cin * len(taps)
        prog.floor_s += max((du.element_size() * (du.numel() + x.numel()) + 4.0 * dw.numel()) / HBM_PEAK_BPS,
                            2.0 * n * ho * wo * cout * cin * len(taps) / MFMA_PEAK_FLOPS)
        if not f32:
            route = 'wgrad8_kernel' if int(fn['cms_conv_wgrad_uses_wgrad8'](C.byref(d))) else 'conv_wgrad_kernel'
            r = prog.by_route.setdefault(route, [0, 0.0, 0.0])
            r[0] += 1; r[1] += du.element_size() * (du.numel() + x.numel()) + 4.0 * dw.numel()
            r[2] += 2.0 * n * ho * wo * cout * cin * len(taps)
        return dw
    name = 'cms_conv_wgrad_f32' if f32 else 'cms_conv_wgrad'
    check(fn[name](C.byref(d), _stream()), name)
    return dw


def channel_sum(src, dst):
    """dst (fp32 [C], accumulated with atomics) += sum over all leading dimensions of src[..., C] (bf16 / fp32, contiguous,
    C % 64 == 0): d(beta) = sum_p dU of a trainable BatchNorm affine over frozen statistics (csrc/wfinish.hip). A program op while
    recording."""
    _need_cuda(src, dst)
    c = int(src.shape[-1])
    if not src.is_contiguous() or src.dtype not in (torch.bfloat16, torch.float32) or dst.dtype != torch.float32 \
            or not dst.is_contiguous() or int(dst.numel()) != c or c % 64:
        raise TypeError('channel_sum: contiguous bf16 / fp32 (..., C) input with C % 64 == 0 and an fp32 [C] output required')
    rows = src.numel() // c
    if _REC is not None:
        prog = _REC[0]
        idx = fn['cms_program_add_channel_sum'](prog.h, _ptr(src), _dtype_code(src), rows, c, _ptr(dst), _rec_stream_index(), prog.group)
        if idx < 0:
            check(idx, 'cms_program_add_channel_sum')
        prog.keep += [src, dst]
        return dst
    check(fn['cms_channel_sum'](_ptr(src), _dtype_code(src), rows, c, _ptr(dst), _stream()), 'cms_channel_sum')
    return dst


def wgrad_finish(items):
    """ONE launch behind the weight gradients of a backward pass whose BatchNorm affine trains over frozen statistics
    (csrc/wfinish.hip): `items` = list of (scratch, grad, w_bf16, scale, wdot) with scratch / grad fp32 (ntaps, Cout, Cin) -- the
    unscaled gradient G the eight-phase kernel wrote and the arena's slice --, w_bf16 the weight in the same layout, scale fp32
    [Cout] or None, wdot fp32 [Cout]: grad += scale * G, wdot += <W, G> per output channel, G cleared. A program op while recording
    (the device-resident item table then belongs to the program)."""
    if not items:
        return
    arr = (_lib.WfinishItem * len(items))()
    keep = []
    for i, (scratch, grad, w, scale, wdot) in enumerate(items):
        _need_cuda(scratch, grad, w, scale, wdot)
        nt, co, ci = (int(v) for v in w.shape)
        if not (scratch.dtype == grad.dtype == wdot.dtype == torch.float32 and w.dtype == torch.bfloat16 and scratch.is_contiguous()
                and grad.is_contiguous() and w.is_contiguous() and tuple(scratch.shape) == tuple(grad.shape) == (nt, co, ci)
                and int(wdot.numel()) == co and wdot.is_contiguous() and ci % 4 == 0
                and (scale is None or (scale.dtype == torch.float32 and int(scale.numel()) == co and scale.is_contiguous()))):
            raise TypeError('wgrad_finish: item {}: fp32 scratch / grad (ntaps, Cout, Cin), bf16 weight of that shape, fp32 [Cout] '
                            'scale / wdot, Cin % 4 == 0 required'.format(i))
        m = arr[i]
        m.scratch, m.grad, m.w, m.wdot = scratch.data_ptr(), grad.data_ptr(), w.data_ptr(), wdot.data_ptr()
        m.scale = scale.data_ptr() if scale is not None else None
        m.ntaps, m.cout, m.cin = nt, co, ci
        keep += [t for t in (scratch, grad, w, scale, wdot) if t is not None]
    total = int(fn['cms_wgrad_finish_pack'](arr, len(items)))
    if total < 0:
        check(total, 'cms_wgrad_finish_pack')
    nbytes = C.sizeof(_lib.WfinishItem) * len(items)
    host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    C.memmove(host.data_ptr(), C.addressof(arr), nbytes)
    dev = items[0][0].device
    table = host.to(dev, non_blocking=True)
    if _REC is not None:
        prog = _REC[0]
        idx = fn['cms_program_add_wgrad_finish'](prog.h, C.c_void_p(table.data_ptr()), len(items), total, _rec_stream_index(), prog.group)
        if idx < 0:
            check(idx, 'cms_program_add_wgrad_finish')
        prog.keep += keep + [table, host]
        torch.cuda.current_stream().synchronize()      # (recorded once: the table is in place before any replay, on whatever stream)
        return
    check(fn['cms_wgrad_finish_run'](C.c_void_p(table.data_ptr()), len(items), total, _stream()), 'cms_wgrad_finish_run')
    table.record_stream(torch.cuda.current_stream())


def conv_wgrad_group(jobs, target_workgroups=0):
    """The weight gradients of MANY layers as one grid per kind (cms_conv_wgrad_group_*): `jobs` = list of
    (du, x, taps, dw, stride, scale) as for `conv_wgrad`. Launches that cannot join a group (channel counts that are not
    multiples of 128, fp32, deterministic slabs) are issued one by one. Under recording the device-resident item tables belong to
    the program. Returns the number of grouped launches."""
    if not jobs:
        return 0
    singles, kinds = [], {1: [], 2: []}
    for job in jobs:
        du, x, taps, dw, stride, scale = job
        _need_cuda(du, x, dw, scale)
        ok = du.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dw.dtype == torch.float32 and du.is_contiguous() \
            and x.is_contiguous() and dw.is_contiguous() and not _WGRAD_DETERMINISTIC and not _WGRAD_SLAB_LARGE
        d = None
        if ok:
            n, ho, wo, cout = (int(v) for v in du.shape)
            n2, h, w_in, cin = (int(v) for v in x.shape)
            if n2 != n or tuple(dw.shape) != (len(taps), cout, cin):
                raise ValueError('conv_wgrad_group: shape mismatch')
            d = _lib.WgradDesc()
            d.du, d.x, d.dw = du.data_ptr(), x.data_ptr(), dw.data_ptr()
            d.scale = scale.data_ptr() if scale is not None else None
            d.n, d.h, d.w_in, d.cin, d.ho, d.wo, d.cout = n, h, w_in, cin, ho, wo, cout
            d.ntaps = len(taps)
            for i, (dy, dx) in enumerate(taps):
                d.tap_dy[i], d.tap_dx[i] = int(dy), int(dx)
            d.stride = int(stride)
            kind = int(fn['cms_conv_wgrad_group_kind'](C.byref(d)))
            if kind in kinds:
                kinds[kind].append((d, job))
                continue
        singles.append(job)
    launched = 0
    for kind, items in kinds.items():
        if len(items) == 1:                    # nothing to group with
            singles.append(items[0][1])
            continue
        if not items:
            continue
        n_items = len(items)
        arr = (_lib.WgradDesc * n_items)(*[d for d, _ in items])
        nbytes = int(fn['cms_conv_wgrad_group_bytes'](n_items))
        host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        total = C.c_int(0)
        check(fn['cms_conv_wgrad_group_pack'](arr, n_items, int(target_workgroups), C.c_void_p(host.data_ptr()), nbytes, C.byref(total)),
              'cms_conv_wgrad_group_pack')
        dev = items[0][1][0].device
        table = host.to(dev, non_blocking=True)
        keep = [table, host] + [t for _, job in items for t in (job[0], job[1], job[3], job[5]) if t is not None]
        if _REC is not None:
            prog = _REC[0]
            idx = fn['cms_program_add_wgrad_group'](prog.h, C.c_void_p(table.data_ptr()), n_items, int(total.value), kind,
                                                   _rec_stream_index(), prog.group)
            if idx < 0:
                check(idx, 'cms_program_add_wgrad_group')
            prog.keep += keep
            for d, (du, x, taps, dw, stride, scale) in items:
                fl = 2.0 * d.n * d.ho * d.wo * d.cout * d.cin * d.ntaps
                prog.flops += fl
                prog.floor_s += max((du.element_size() * (du.numel() + x.numel()) + 4.0 * dw.numel()) / HBM_PEAK_BPS,
                                    fl / MFMA_PEAK_FLOPS)
        else:
            check(fn['cms_conv_wgrad_group_run'](C.c_void_p(table.data_ptr()), n_items, int(total.value), kind, _stream()),
                  'cms_conv_wgrad_group_run')
            table.record_stream(torch.cuda.current_stream())
        launched += 1
    for du, x, taps, dw, stride, scale in singles:
        conv_wgrad(du, x, taps, dw, stride=stride, scale=scale)
    return launched
