"""
Test infrastructure: the unsupervised branch of the reference's augmentation mean-teacher trainer restated with torch on the
CPU (train_seg_semisup_aug_mt.py:302-397 of the upstream repository), statement by statement; gradients come from autograd.
`F.affine_grid`, `F.grid_sample`, `F.softmax`, `F.log_softmax`, `F.kl_div`, `F.smooth_l1_loss` and `F.interpolate` are the
ATen CPU ops the reference calls. The tensors' dtype decides the precision (float32 as the reference runs, float64 for the
error budget).

One deliberate difference: the reference's `logits_var` branch (:370-374) overwrites its result with
`delta_prob * delta_prob` where `delta_prob` is unassigned, so it raises; the evident intent, sum_c (delta logits)^2 / sqrt(C)
as in the CutMix trainer, is what is restated here.
"""
import math

import torch
import torch.nn.functional as F

from oracle.losses import upsample

LOSS_FNS = ('var', 'logits_var', 'logits_smoothl1', 'bce', 'kld')
AFFINE_KW = dict(align_corners=True)          # datapipe/torch_utils.py: affine_align_corners_kw(True)


def robust_binary_crossentropy(pred, tgt, eps=1e-6):
    """architectures/network_architectures.py:115-118"""
    inv_tgt = 1.0 - tgt
    inv_pred = 1.0 - pred + eps
    return -(tgt * torch.log(pred + eps) + inv_tgt * torch.log(inv_pred))


def warp_grid(xf0_to_1, shape):
    """:302"""
    return F.affine_grid(xf0_to_1, list(shape), **AFFINE_KW)


def warped_confidence(logits_cons_tea, xf0_to_1):
    """:309, 312, 347 -> (N,H,W)"""
    grid = warp_grid(xf0_to_1, logits_cons_tea.shape)
    prob = F.grid_sample(F.softmax(logits_cons_tea, dim=1), grid, **AFFINE_KW)
    return prob.max(dim=1)[0]


def aug_unsup_loss(logits_cons_stu, logits_cons_tea, batch_ufx0_to_1, batch_um0, batch_um1, cons_loss_fn='var',
                   conf_thresh=0.97, conf_per_pixel=False, ramp_val=1.0, rampup=-1, cons_weight=1.0):
    """Full-resolution logits in. -> dict(consistency_loss=<the logged value, :400>, unsup_loss=<what is back-propagated, :397>,
    conf_rate=<:351, None without a threshold>)."""
    n_classes = logits_cons_stu.shape[1]
    root_n_classes = math.sqrt(n_classes)
    logits_cons_tea = logits_cons_tea.detach()
    grid_tea_to_stu = warp_grid(batch_ufx0_to_1, logits_cons_tea.shape)                                     # :302
    logits_cons_tea_in_stu = F.grid_sample(logits_cons_tea, grid_tea_to_stu, **AFFINE_KW)                   # :304
    mask_tea_in_stu = F.grid_sample(batch_um0, grid_tea_to_stu, **AFFINE_KW) * batch_um1                    # :306
    prob_cons_tea = F.softmax(logits_cons_tea, dim=1)                                                       # :309-312
    prob_cons_stu = F.softmax(logits_cons_stu, dim=1)
    prob_cons_tea_in_stu = F.grid_sample(prob_cons_tea, grid_tea_to_stu, **AFFINE_KW)

    loss_mask = mask_tea_in_stu
    conf_rate = None
    if conf_thresh > 0.0:                                                                                   # :345-356
        conf_tea = prob_cons_tea_in_stu.max(dim=1)[0]
        conf_mask = (conf_tea >= conf_thresh).to(logits_cons_stu.dtype)[:, None, :, :]
        conf_rate = float(conf_mask.mean())
        if not conf_per_pixel:
            conf_mask = conf_mask.mean()
        loss_mask = loss_mask * conf_mask

    if cons_loss_fn == 'var':                                                                               # :366-387
        delta_prob = prob_cons_stu - prob_cons_tea_in_stu
        consistency_loss = (delta_prob * delta_prob).sum(dim=1, keepdim=True)
    elif cons_loss_fn == 'logits_var':
        delta_logits = logits_cons_stu - logits_cons_tea_in_stu
        consistency_loss = (delta_logits * delta_logits).sum(dim=1, keepdim=True) / root_n_classes
    elif cons_loss_fn == 'logits_smoothl1':
        consistency_loss = F.smooth_l1_loss(logits_cons_stu, logits_cons_tea_in_stu, reduction='none')
        consistency_loss = consistency_loss.sum(dim=1, keepdim=True) / root_n_classes
    elif cons_loss_fn == 'bce':
        consistency_loss = robust_binary_crossentropy(prob_cons_stu, prob_cons_tea_in_stu).sum(dim=1, keepdim=True)
    elif cons_loss_fn == 'kld':
        consistency_loss = F.kl_div(F.log_softmax(logits_cons_stu, dim=1), prob_cons_tea_in_stu, reduction='none')
        consistency_loss = consistency_loss.sum(dim=1, keepdim=True)
    else:
        raise ValueError('Unknown consistency loss function {}'.format(cons_loss_fn))

    consistency_loss = (consistency_loss * loss_mask).mean()                                                # :390
    if rampup > 0:
        consistency_loss = consistency_loss * ramp_val
    unsup_loss = consistency_loss * cons_weight
    return dict(consistency_loss=consistency_loss, unsup_loss=unsup_loss, conf_rate=conf_rate)


def aug_from_lowres(l_stu, l_tea, xf0_to_1, um0, um1, out_size, align_corners, dtype=torch.float32, **kw):
    """Low-resolution logits in (the networks upsample inside `forward`). -> (result dict, gradient of unsup_loss wrt l_stu, the
    warped confidence (N,H,W))."""
    H, W = int(out_size[0]), int(out_size[1])
    n = l_stu.shape[0]
    ones = torch.ones(n, 1, H, W, dtype=dtype)
    um0 = ones if um0 is None else um0.to(dtype)
    um1 = ones if um1 is None else um1.to(dtype)
    xf = torch.as_tensor(xf0_to_1).to(dtype)
    ls = l_stu.detach().to(dtype).clone().requires_grad_(True)
    up = lambda t: upsample(t, (H, W), align_corners=align_corners)
    LT = up(l_tea.detach().to(dtype))
    r = aug_unsup_loss(up(ls), LT, xf, um0, um1, **kw)
    r['unsup_loss'].backward()
    return r, ls.grad, warped_confidence(LT, xf)


# ---- geometry helpers of the tests
def theta_from_pixel_affine(A, H, W):
    """A pixel-space map (N,2,3) (x_src, y_src) = A [x_dst, y_dst, 1] -> the theta of F.affine_grid(align_corners=True) that
    samples the same positions: the inverse of the fold in ops.aug_pixel_matrices, in float64."""
    A = torch.as_tensor(A, dtype=torch.float64)
    rx, ry = (W - 1) / 2.0, (H - 1) / 2.0
    t = torch.zeros_like(A)
    t[:, 0, 0] = A[:, 0, 0]
    t[:, 0, 1] = A[:, 0, 1] * (ry / rx)
    t[:, 0, 2] = A[:, 0, 2] / rx + t[:, 0, 0] + t[:, 0, 1] - 1.0
    t[:, 1, 0] = A[:, 1, 0] * (rx / ry)
    t[:, 1, 1] = A[:, 1, 1]
    t[:, 1, 2] = A[:, 1, 2] / ry + t[:, 1, 0] + t[:, 1, 1] - 1.0
    return t


def rot_scale_theta(deg, scale, tx=0.0, ty=0.0):
    """theta (2,3) in normalised coordinates: rotation by `deg` about the centre, zoom `scale`, translation (tx, ty)"""
    r = math.radians(deg)
    c, s = math.cos(r) * scale, math.sin(r) * scale
    return [[c, -s, tx], [s, c, ty]]


# ---- tile facts: which route (teacher rectangle staged in LDS / gathered from global memory) the kernels take -----------------
# A restatement of the host-side capacity rule of csrc/aug_loss.hip and csrc/loss_tiles.hpp (aug_tea_cap, fwd_tiles, tile_lds_bytes) and of the
# per-workgroup decision (aug_tile_patch + aug_fits). The tile's box of teacher pixels comes from the product's own
# aug_tile_box through tests/hostcheck_aug (`hc`), the rest is restated here with numpy float32 arithmetic.
TILE_W, FWD_TILE_H, BWD_TILE_H = 64, 8, 4
FWD_PATCH_LDS_MAX, BWD_LDS_MAX, AUG_TEA_LDS_MAX = 96 * 1024, 160 * 1024 - 4096, 32 * 1024


def _f(v):
    import numpy as np
    return np.float32(v)


def bilin_scale(n_in, n_out, align):
    if align:
        return _f(n_in - 1) / _f(n_out - 1) if n_out > 1 else _f(0)
    return _f(n_in) / _f(n_out)


def bilin_cells(dst, scale, n_in, align):
    """(i0, i1) of pixel_math.hpp's bilin_tap"""
    if align:
        src = scale * _f(dst)
    else:
        src = max(scale * (_f(dst) + _f(0.5)) - _f(0.5), _f(0))
    i0 = min(int(src), n_in - 1)
    return i0, i0 + (1 if i0 < n_in - 1 else 0)


def tea_capacity(C, lo, hi, align, backward):
    """floats of LDS the teacher's rectangle may use; None: the launch does not use the tiled kernel at all"""
    (h, w), (H, W) = lo, hi
    if (h, w) == (H, W):
        return None
    sy, sx = bilin_scale(h, H, align), bilin_scale(w, W, align)
    cols = int(_f(TILE_W - 1) * sx) + 3
    rows = lambda th: int(_f(th - 1) * sy) + 3
    if backward:
        used = (BWD_TILE_H * C * (TILE_W + 1) + BWD_TILE_H * C * cols + C * rows(BWD_TILE_H) * cols) * 4
        limit = BWD_LDS_MAX
        assert used <= limit
    else:
        used = C * rows(FWD_TILE_H) * cols * 4
        limit = FWD_PATCH_LDS_MAX
        if used > limit:
            return None
    return min(limit - used, AUG_TEA_LDS_MAX) // 4


def tile_facts(hc, xf_pixels, C, lo, hi, align, backward):
    """-> dict(staged=, global_=, outside=, max_floats=): the number of (sample, tile) workgroups per route"""
    import ctypes
    import numpy as np
    (h, w), (H, W) = lo, hi
    cap = tea_capacity(C, lo, hi, align, backward)
    assert cap is not None
    sy, sx = bilin_scale(h, H, align), bilin_scale(w, W, align)
    th_full = BWD_TILE_H if backward else FWD_TILE_H
    facts = dict(staged=0, global_=0, outside=0, max_floats=0, cap=cap)
    box = (ctypes.c_int * 4)()
    for row in np.ascontiguousarray(xf_pixels, dtype=np.float32):
        for y0 in range(0, H, th_full):
            for x0 in range(0, W, TILE_W):
                tw, th = min(TILE_W, W - x0), min(th_full, H - y0)
                hc.hc_aug_tile_box(row.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), x0, y0, tw, th, H, W, box)
                x_lo, x_hi, y_lo, y_hi = box
                if x_hi < x_lo or y_hi < y_lo:
                    facts['outside'] += 1
                    continue
                n_cols = bilin_cells(x_hi, sx, w, align)[1] - bilin_cells(x_lo, sx, w, align)[0] + 1
                n_rows = bilin_cells(y_hi, sy, h, align)[1] - bilin_cells(y_lo, sy, h, align)[0] + 1
                floats = C * n_rows * n_cols
                facts['max_floats'] = max(facts['max_floats'], floats)
                facts['staged' if floats <= cap else 'global_'] += 1
    return facts
