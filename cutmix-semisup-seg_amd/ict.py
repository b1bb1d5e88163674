"""
Interpolation consistency training (ICT) mean-teacher iteration -- the body of the reference's third trainer,
train_seg_semisup_ict.py:249-403.

    student(x_sup) -> CE -> backward                                                    :261-263
    lambda ~ Beta(ict_alpha, ict_alpha) per sample                                      :306-307
    x_mix = x0_stu*(1-lambda) + x1_stu*lambda                                           :310
    teacher(x0_tea), teacher(x1_tea) (no grad), student(x_mix)                          :314-318
    consistency between student(x_mix) and the same blend of the teacher's predictions  :320-391
    optimizer + EMA                                                                     :397-399

What runs where: the network passes, the cross entropy and Adam/SGD + EMA are the MI355X kernels of the CutMix step
(step.py); the image blend and the interpolation loss are both csrc/ict.hip (arithmetic in csrc/ict_math.hpp). The validity
masks are blended inside the loss kernels (:311 never becomes a tensor). The mix factors are drawn on the host with the
reference's own call (numpy's Beta sampler) and travel to the device as N floats.

First version: eager launches (no hipGraph capture), one GPU.
"""
import os

import numpy as np
import torch

from . import ops
from .step import step_result, supervised_pass, world_size


class ICTConfig(object):
    def __init__(self, ict_alpha=0.1, cons_loss_fn='var', cons_weight=0.3, conf_thresh=0.97, conf_per_pixel=False, rampup=-1,
                 unsup_batch_ratio=1):
        self.ict_alpha = float(ict_alpha)
        self.cons_loss_fn = cons_loss_fn
        self.cons_weight = float(cons_weight)
        self.rampup = rampup
        self.unsup_batch_ratio = int(unsup_batch_ratio)
        self.cons = ops.ICTConsistencyConfig(loss_fn=cons_loss_fn, conf_thresh=conf_thresh, conf_per_pixel=conf_per_pixel)


class ICTUnsupBatch(object):
    """Two unsupervised batches (:272-291). x*_tea: the teacher's (weakly augmented) images; x*_stu: the student's (strongly
    augmented) ones, the teacher's when not given; um*: validity masks (N,1,H,W) or None (all valid)."""

    def __init__(self, x0_tea, x1_tea, um0=None, um1=None, x0_stu=None, x1_stu=None):
        self.x0_tea, self.x1_tea = x0_tea, x1_tea
        self.um0, self.um1 = um0, um1
        self.x0_stu = x0_tea if x0_stu is None else x0_stu
        self.x1_stu = x1_tea if x1_stu is None else x1_stu


class ICTMeanTeacherStep(object):
    def __init__(self, student_net, teacher_net, student_optim, teacher_optim, cfg, rng=None):
        if world_size(None) > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise RuntimeError('ICTMeanTeacherStep runs on one GPU: data-parallel ICT (gradient exchange, global confidence '
                               'rate) is not implemented')
        self.student, self.teacher = student_net, teacher_net
        self.student_optim, self.teacher_optim = student_optim, teacher_optim
        self.cfg = cfg
        self.rng = np.random if rng is None else rng          # the reference draws from numpy's global state (:306)
        self.align_corners = getattr(student_net, 'upsample_align_corners', True)
        cfg.cons.align_corners = self.align_corners

    def draw_lam(self, n, device):
        """:306-307 -> f32 (N,) on the device (through pinned memory, see ops.ranges_to_device)"""
        lam = self.rng.beta(self.cfg.ict_alpha, self.cfg.ict_alpha, size=(n, 1, 1, 1))
        lam = torch.tensor(lam, dtype=torch.float).reshape(-1)
        return lam.pin_memory().to(device, non_blocking=True)

    def __call__(self, sup_x, sup_y, unsup_batches, ramp_val=1.0, lam=None):
        """`lam` (optional): the mix factors, one (N,) tensor for every unsupervised batch or a list with one per batch (tests
        inject the reference's draw)."""
        cfg = self.cfg
        ramp = ramp_val if cfg.rampup > 0 else 1.0
        out_size = sup_x.shape[2:4]
        self.student_optim.zero_grad()
        ce_sc = supervised_pass(self.student, sup_x, sup_y, out_size, self.align_corners, None)
        cons_vals = []
        if cfg.cons_weight > 0.0:
            for bi, ub in enumerate(unsup_batches):
                n = int(ub.x0_tea.shape[0])
                if lam is None:
                    lam_b = self.draw_lam(n, ub.x0_tea.device)
                else:
                    lam_b = lam[bi] if isinstance(lam, (list, tuple)) else lam
                    lam_b = lam_b.to(device=ub.x0_tea.device, dtype=torch.float32).reshape(-1)
                x_mix = ops.ict_blend(ub.x0_stu, ub.x1_stu, lam_b)
                with torch.no_grad():
                    l_tea0 = self.teacher.forward_lowres(ub.x0_tea)
                    l_tea1 = self.teacher.forward_lowres(ub.x1_tea)
                l_stu = self.student.forward_lowres(x_mix)
                sc, cctx = ops.ict_consistency_forward(cfg.cons, l_stu.detach(), l_tea0, l_tea1, lam_b, out_size, um0=ub.um0,
                                                       um1=ub.um1, ramp_val=ramp, cons_weight=cfg.cons_weight)
                l_stu.backward(ops.ict_consistency_backward(cctx, sc).to(l_stu.dtype))
                cons_vals.append(sc)
        ops.join_side_streams()
        self.student_optim.step()
        if self.teacher_optim is not None:
            self.teacher_optim.step()
        return step_result(ce_sc, cons_vals)
