"""
Cross pseudo supervision (CPS) with CutMix -- Chen, Yuan, Zeng, Wang, "Semi-Supervised Semantic Segmentation with Cross Pseudo
Supervision", CVPR 2021 -- as one iteration on one GPU. The reference this project mirrors has no such trainer, and the authors'
code was not at hand when this was written: the definition below is the paper's as recalled and is THIS PROJECT'S definition
(include/cutmixseg.h, DESIGN 8, tests/_cps_refs.py pin it).

Two networks a and b of one architecture, initialised differently; no teacher, no EMA. Per unsupervised batch (step.UnsupBatch:
x0_tea, x1_tea, x0_stu, x1_stu, um0, um1 and exactly one of ranges / mask):

    L0_k = net_k(x0_tea), L1_k = net_k(x1_tea)            under no_grad, in training mode, k = a, b
    label_a, label_b = ops.cps_labels(L0_a, L1_a, L0_b, L1_b, ...)     hard labels of the mixed pair, 255 where invalid or unsure
    x_mix = ops.cutmix_paste(x0_stu, x1_stu, ...)         the same mask
    loss_a = CE(net_a(x_mix), label_b), loss_b = CE(net_b(x_mix), label_a)       ignore_index 255, mean over the kept pixels
    both backwards with loss_weight = cons_weight * ramp

plus the supervised cross entropy on each network, then both optimisers. What runs where: the network passes, the cross entropy and
Adam / SGD are the MI355X kernels of the CutMix step (step.py); the labels are ONE launch of csrc/cps.hip (arithmetic in
csrc/cps_math.hpp) that shares the mask bit, the validity and the bilinear taps of a pixel between the two networks.

Eager launches (no hipGraph capture, no batch fusion), one GPU.
"""
import os

import torch

from . import ops
from .step import supervised_pass, world_size


def align_corners(net):
    """the corner convention of a network's upsample (DeepLab v2: True, the others say)"""
    return bool(getattr(net, 'upsample_align_corners', True))


class CPSConfig(object):
    def __init__(self, cons_weight=1.5, conf_thresh=0.0, rampup=-1, unsup_batch_ratio=1, invert=True):
        self.cons_weight = float(cons_weight)
        self.conf_thresh = float(conf_thresh)
        self.rampup = rampup
        self.unsup_batch_ratio = int(unsup_batch_ratio)
        self.invert = bool(invert)


class CrossPseudoStep(object):
    def __init__(self, net_a, net_b, optim_a, optim_b, cfg):
        if world_size(None) > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise RuntimeError('CrossPseudoStep runs on one GPU: data-parallel CPS (gradient exchange, global label counts) is not '
                               'implemented')
        if net_a is net_b:
            raise ValueError('CrossPseudoStep: the two networks are one object')
        if align_corners(net_a) != align_corners(net_b):
            raise ValueError('CrossPseudoStep: the two networks upsample with different corner conventions')
        self.net_a, self.net_b = net_a, net_b
        self.optim_a, self.optim_b = optim_a, optim_b
        self.cfg = cfg
        self.align_corners = align_corners(net_a)
        self.last_labels = None        # (label_a, label_b, stats) of the last unsupervised batch: tests and tools read them
        self._agree = None             # device f64[2]: the sum of the batches' agreement since pop_agreement(), and their number

    def pop_agreement(self):
        """the mean pseudo-label agreement of the unsupervised batches since the last call (one host synchronisation), None when
        there were none"""
        acc, self._agree = self._agree, None
        if acc is None:
            return None
        total, count = acc.cpu().tolist()
        return total / count if count > 0 else None

    def _direction(self, net, x_mix, labels, kept, out_size, weight):
        """CE(net(x_mix), labels) -> backward; the loss, 0 where the other network kept no label (the gradient is zero already: the
        finaliser's factor is 0 there). No host synchronisation."""
        s = net.forward_lowres(x_mix)
        sc, ctx = ops.ce_forward(s.detach(), labels, out_size, 255, self.align_corners, loss_weight=weight)
        s.backward(ops.ce_backward(ctx, sc).to(s.dtype))
        return torch.where(kept > 0, sc[0], torch.zeros_like(sc[0]))

    def __call__(self, sup_x, sup_y, unsup_batches, ramp_val=1.0):
        cfg = self.cfg
        ramp = ramp_val if cfg.rampup > 0 else 1.0
        out_size = tuple(int(v) for v in sup_x.shape[2:4])
        self.optim_a.zero_grad()
        self.optim_b.zero_grad()
        ce_a = supervised_pass(self.net_a, sup_x, sup_y, out_size, self.align_corners, None)
        ce_b = supervised_pass(self.net_b, sup_x, sup_y, out_size, self.align_corners, None)
        res = dict(sup_loss=(ce_a[0] + ce_b[0]) * 0.5, consistency_loss=None, conf_rate=None, agreement=None)
        cons, rates, agrees = [], [], []
        if cfg.cons_weight > 0.0:
            for ub in unsup_batches:
                if (ub.ranges is None) == (ub.mask is None):
                    raise ValueError('CrossPseudoStep: an unsupervised batch needs exactly one of ranges / mask')
                with torch.no_grad():
                    l0_a, l1_a = self.net_a.forward_lowres(ub.x0_tea), self.net_a.forward_lowres(ub.x1_tea)
                    l0_b, l1_b = self.net_b.forward_lowres(ub.x0_tea), self.net_b.forward_lowres(ub.x1_tea)
                label_a, label_b, stats = ops.cps_labels(l0_a, l1_a, l0_b, l1_b, out_size, ranges=ub.ranges, mask=ub.mask,
                                                         invert=cfg.invert, um0=ub.um0, um1=ub.um1, conf_thresh=cfg.conf_thresh,
                                                         align_corners=self.align_corners)
                self.last_labels = (label_a, label_b, stats)
                x_mix = ops.cutmix_paste(ub.x0_stu, ub.x1_stu, ranges=ub.ranges, invert=cfg.invert, mask=ub.mask)
                weight = cfg.cons_weight * ramp
                loss_a = self._direction(self.net_a, x_mix, label_b, stats[2], out_size, weight)
                loss_b = self._direction(self.net_b, x_mix, label_a, stats[1], out_size, weight)
                cons.append((loss_a + loss_b) * ramp)
                st = stats.to(torch.float64)
                rates.append((st[1] + st[2]) / (2.0 * label_a.numel()))
                agrees.append(st[3] / torch.clamp(st[0], min=1.0))
        ops.join_side_streams()
        self.optim_a.step()
        self.optim_b.step()
        if cons:
            res['consistency_loss'] = torch.stack(cons).mean()
            res['conf_rate'] = torch.stack(rates).mean().to(torch.float32)
            res['agreement'] = torch.stack(agrees).mean().to(torch.float32)
            if self._agree is None:
                self._agree = torch.zeros(2, dtype=torch.float64, device=sup_x.device)
            self._agree[0] += torch.stack(agrees).sum()
            self._agree[1] += len(agrees)
        return res
