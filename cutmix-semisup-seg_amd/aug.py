"""
Augmentation-consistency mean-teacher iteration -- the body of the reference's fourth trainer,
train_seg_semisup_aug_mt.py:250-410, the classic mean teacher between two differently augmented views of the same images.

    student(x_sup) -> CE -> backward                                                    :260-265
    teacher(view 0) (no grad), student(view 1)                                          :296-299
    the teacher's prediction warped into the student's view by xf0_to_1                 :302-312
    consistency between the two, masked by the warped validity mask x view 1's          :341-398
    optimizer + EMA                                                                     :404-406

What runs where: the network passes, the cross entropy and Adam/SGD + EMA are the MI355X kernels of the CutMix step (step.py);
the warp and the loss are ONE pair of launches, csrc/aug_loss.hip (arithmetic in csrc/aug_math.hpp):
no F.affine_grid / F.grid_sample, no warped (N,C,H,W) tensor. The pair geometry (xf0_to_1) comes with the batch, as in the
reference's loader; aug_pairs.py draws it for synthetic data.

First version: eager launches (no hipGraph capture), one GPU.
"""
import os

import torch

from . import ops
from .step import step_result, supervised_pass, world_size


class AugConfig(object):
    def __init__(self, cons_loss_fn='var', cons_weight=1.0, conf_thresh=0.97, conf_per_pixel=False, rampup=-1, unsup_batch_ratio=1):
        self.cons_loss_fn = cons_loss_fn
        self.cons_weight = float(cons_weight)
        self.rampup = rampup
        self.unsup_batch_ratio = int(unsup_batch_ratio)
        self.cons = ops.AugConsistencyConfig(loss_fn=cons_loss_fn, conf_thresh=conf_thresh, conf_per_pixel=conf_per_pixel)


class AugUnsupBatch(object):
    """A pair of views (:277-281). x0: the teacher's view, x1: the student's; xf0_to_1 (N,2,3): the theta of
    F.affine_grid(align_corners=True) that warps view 0 into view 1 (numpy, CPU or device tensor); um*: validity masks
    (N,1,H,W) or None (all valid)."""

    def __init__(self, x0, x1, xf0_to_1, um0=None, um1=None):
        self.x0, self.x1, self.xf0_to_1 = x0, x1, xf0_to_1
        self.um0, self.um1 = um0, um1


class AugMeanTeacherStep(object):
    def __init__(self, student_net, teacher_net, student_optim, teacher_optim, cfg):
        if world_size(None) > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise RuntimeError('AugMeanTeacherStep runs on one GPU: data-parallel augmentation consistency (gradient exchange, '
                               'global confidence rate) is not implemented')
        self.student, self.teacher = student_net, teacher_net           # model='pi': teacher_net is student_net
        self.student_optim, self.teacher_optim = student_optim, teacher_optim
        self.cfg = cfg
        self.align_corners = getattr(student_net, 'upsample_align_corners', True)
        cfg.cons.align_corners = self.align_corners

    def __call__(self, sup_x, sup_y, unsup_batches, ramp_val=1.0):
        cfg = self.cfg
        ramp = ramp_val if cfg.rampup > 0 else 1.0
        out_size = sup_x.shape[2:4]
        self.student_optim.zero_grad()
        ce_sc = supervised_pass(self.student, sup_x, sup_y, out_size, self.align_corners, None)
        cons_vals = []
        if cfg.cons_weight > 0.0:
            for ub in unsup_batches:
                with torch.no_grad():
                    l_tea = self.teacher.forward_lowres(ub.x0)
                l_stu = self.student.forward_lowres(ub.x1)
                sc, cctx = ops.aug_consistency_forward(cfg.cons, l_stu.detach(), l_tea.detach(), ub.xf0_to_1, ub.x1.shape[2:4],
                                                       um0=ub.um0, um1=ub.um1, ramp_val=ramp, cons_weight=cfg.cons_weight)
                l_stu.backward(ops.aug_consistency_backward(cctx, sc).to(l_stu.dtype))
                cons_vals.append(sc)
        ops.join_side_streams()
        self.student_optim.step()
        if self.teacher_optim is not None:
            self.teacher_optim.step()
        return step_result(ce_sc, cons_vals)
