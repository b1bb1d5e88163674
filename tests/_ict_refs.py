"""
Test infrastructure: the unsupervised branch of the reference's ICT trainer restated with torch on the CPU
(train_seg_semisup_ict.py:306-391 of the upstream repository), statement by statement; gradients come from autograd.
`F.softmax`, `F.log_softmax`, `F.kl_div`, `F.smooth_l1_loss` and `F.interpolate` are the ATen CPU ops the reference
calls. The `--conf_per_pixel` mask is built exactly as :343 builds it -- `[:, None, :, :]` on a tensor that already
carries the channel axis, (N,1,1,H,W), broadcast against the (N,1,H,W) loss to (N,N,1,H,W) -- NOT in the simplified
batch-mean form the kernels use, so that the simplification is what the comparison tests.
"""
import math

import torch
import torch.nn.functional as F

from oracle.losses import upsample

LOSS_FNS = ('var', 'logits_var', 'logits_smoothl1', 'bce', 'kld')


def robust_binary_crossentropy(pred, tgt, eps=1e-6):
    """architectures/network_architectures.py:115-118"""
    inv_tgt = 1.0 - tgt
    inv_pred = 1.0 - pred + eps
    return -(tgt * torch.log(pred + eps) + inv_tgt * torch.log(inv_pred))


def mix_factors(lam):
    """(N,) -> float32 (N,1,1,1), the shape of :306-307"""
    return torch.as_tensor(lam, dtype=torch.float32).reshape(-1, 1, 1, 1)


def blend(x0, x1, lam):
    """:310-311"""
    f = mix_factors(lam)
    return x0 * (1.0 - f) + x1 * f


def blended_confidence(logits_u0_tea, logits_u1_tea, lam):
    """:336-341 -> (N,1,H,W)"""
    f = mix_factors(lam)
    conf_u0_tea = F.softmax(logits_u0_tea, dim=1).max(dim=1, keepdim=True)[0]
    conf_u1_tea = F.softmax(logits_u1_tea, dim=1).max(dim=1, keepdim=True)[0]
    return conf_u0_tea * (1 - f) + conf_u1_tea * f


def ict_unsup_loss(logits_cons_stu, logits_u0_tea, logits_u1_tea, lam, batch_um0, batch_um1, cons_loss_fn='var',
                   conf_thresh=0.97, conf_per_pixel=False, ramp_val=1.0, rampup=-1, cons_weight=0.3):
    """Full-resolution logits in. -> dict(consistency_loss=<the logged value, :393>, unsup_loss=<what is back-propagated, :390>,
    conf_rate=<:345, None without a threshold>)."""
    ict_mix_factors = mix_factors(lam)
    n_classes = logits_cons_stu.shape[1]
    root_n_classes = math.sqrt(n_classes)
    batch_um_mixed = batch_um0 * (1.0 - ict_mix_factors) + batch_um1 * ict_mix_factors                 # :311
    logits_u0_tea, logits_u1_tea = logits_u0_tea.detach(), logits_u1_tea.detach()

    prob_u0_tea = F.softmax(logits_u0_tea, dim=1)                                                       # :321-323
    prob_u1_tea = F.softmax(logits_u1_tea, dim=1)
    prob_cons_stu = F.softmax(logits_cons_stu, dim=1)
    logits_cons_tea = logits_u0_tea * (1 - ict_mix_factors) + logits_u1_tea * ict_mix_factors           # :328-329
    prob_cons_tea = prob_u0_tea * (1 - ict_mix_factors) + prob_u1_tea * ict_mix_factors

    loss_mask = batch_um_mixed
    conf_rate = None
    if conf_thresh > 0.0:                                                                               # :334-350
        conf_tea = blended_confidence(logits_u0_tea, logits_u1_tea, lam)
        conf_mask = (conf_tea >= conf_thresh).float()[:, None, :, :]
        conf_rate = float(conf_mask.mean())
        if not conf_per_pixel:
            conf_mask = conf_mask.mean()
        loss_mask = loss_mask * conf_mask

    if cons_loss_fn == 'var':                                                                           # :360-380
        delta_prob = prob_cons_stu - prob_cons_tea
        consistency_loss = (delta_prob * delta_prob).sum(dim=1, keepdim=True)
    elif cons_loss_fn == 'logits_var':
        delta_logits = logits_cons_stu - logits_cons_tea
        consistency_loss = (delta_logits * delta_logits).sum(dim=1, keepdim=True) / root_n_classes
    elif cons_loss_fn == 'logits_smoothl1':
        consistency_loss = F.smooth_l1_loss(logits_cons_stu, logits_cons_tea, reduction='none')
        consistency_loss = consistency_loss.sum(dim=1, keepdim=True) / root_n_classes
    elif cons_loss_fn == 'bce':
        consistency_loss = robust_binary_crossentropy(prob_cons_stu, prob_cons_tea).sum(dim=1, keepdim=True)
    elif cons_loss_fn == 'kld':
        consistency_loss = F.kl_div(F.log_softmax(logits_cons_stu, dim=1), prob_cons_tea, reduction='none')
        consistency_loss = consistency_loss.sum(dim=1, keepdim=True)
    else:
        raise ValueError('Unknown consistency loss function {}'.format(cons_loss_fn))

    consistency_loss = (consistency_loss * loss_mask).mean()                                            # :383
    if rampup > 0:
        consistency_loss = consistency_loss * ramp_val
    unsup_loss = consistency_loss * cons_weight
    return dict(consistency_loss=consistency_loss, unsup_loss=unsup_loss, conf_rate=conf_rate)


def ict_from_lowres(l_stu, l_tea0, l_tea1, lam, um0, um1, out_size, align_corners, **kw):
    """Low-resolution logits in (the networks upsample inside `forward`). -> (result dict, gradient of unsup_loss wrt l_stu, the
    blended confidence (N,1,H,W))."""
    H, W = int(out_size[0]), int(out_size[1])
    n = l_stu.shape[0]
    ones = torch.ones(n, 1, H, W)
    um0 = ones if um0 is None else um0
    um1 = ones if um1 is None else um1
    ls = l_stu.detach().clone().requires_grad_(True)
    up = lambda t: upsample(t, (H, W), align_corners=align_corners)
    L0, L1 = up(l_tea0), up(l_tea1)
    r = ict_unsup_loss(up(ls), L0, L1, lam, um0, um1, **kw)
    r['unsup_loss'].backward()
    return r, ls.grad, blended_confidence(L0, L1, lam)
