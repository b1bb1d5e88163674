"""The fused ICT loss (ops.ict_consistency_forward + ict_consistency_backward: csrc/ict_math.hpp,
csrc/ict.hip) at the Pascal configuration's geometry -- logits 10 x 21 x 41 x 41, loss at 321 x 321 -- against the same loss
written with torch ops on the device: materialised bilinear upsamples of the three logit tensors, three softmaxes, the blends, the
masked mean and autograd back to the low-resolution student logits (train_seg_semisup_ict.py:320-391 as the reference runs it).
Both legs run in one process, alternated round by round after warm-up; a leg's time is the host clock around `calls` forward +
backward calls that end in a device synchronise. Prints per-round times, then one JSON line with the medians, the spread (max - min
over the rounds of each leg) and the bytes the fused path must move.
    python tools/ict_loss_bench.py [--rounds 7] [--calls 200] [--warmup 3] [--loss_fn var] [--conf_per_pixel]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cutmix_semisup_seg_amd import ops  # noqa: E402

N, C, h, w, H, W = 10, 21, 41, 41, 321, 321
TAU, WEIGHT = 0.6, 0.3


def compulsory_bytes(conf_per_pixel):
    """what one forward + backward of the fused path has to move through HBM / L2: the three low-resolution logit tensors (read
    by both launches, by the map launch too), the two validity masks (both launches), the gradient rows (zero-fill + atomics:
    write, read, write) and, with --conf_per_pixel, the (H,W) map (written once, read twice)"""
    lo = N * C * h * w * 4
    um = N * H * W * 4
    b = 2 * 3 * lo + 2 * 2 * um + 3 * lo
    if conf_per_pixel:
        b += 2 * lo + 3 * H * W * 4
    return b


def torch_leg(ls, l0, l1, lam, um0, um1, loss_fn, conf_per_pixel):
    """forward + backward with torch ops (var / kld / logits_var; the default confidence mode or the reference's broadcast)"""
    ls = ls.detach().requires_grad_(True)
    f = lam.reshape(-1, 1, 1, 1)
    up = lambda t: F.interpolate(t, size=(H, W), mode='bilinear', align_corners=True)       # noqa: E731
    Ls, L0, L1 = up(ls), up(l0), up(l1)
    p0, p1 = F.softmax(L0, dim=1), F.softmax(L1, dim=1)
    pt = p0 * (1 - f) + p1 * f
    um = um0 * (1.0 - f) + um1 * f
    conf = p0.max(dim=1, keepdim=True)[0] * (1 - f) + p1.max(dim=1, keepdim=True)[0] * f
    cm = (conf >= TAU).float()[:, None, :, :]
    rate = cm.mean()
    mask = um * (cm if conf_per_pixel else rate)
    if loss_fn == 'var':
        d = F.softmax(Ls, dim=1) - pt
        pix = (d * d).sum(dim=1, keepdim=True)
    elif loss_fn == 'kld':
        pix = F.kl_div(F.log_softmax(Ls, dim=1), pt, reduction='none').sum(dim=1, keepdim=True)
    else:
        d = Ls - (L0 * (1 - f) + L1 * f)
        pix = (d * d).sum(dim=1, keepdim=True) / C ** 0.5
    closs = (pix * mask).mean()
    (closs * WEIGHT).backward()
    return closs.detach(), rate, ls.grad


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3        # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--loss_fn', choices=['var', 'kld', 'logits_var'], default='var')
    ap.add_argument('--conf_per_pixel', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ict_loss_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    ls = (torch.randn(N, C, h, w, generator=gen) * 2).to(dev)
    l0 = (torch.randn(N, C, h, w, generator=gen) * 3).to(dev)
    l1 = (torch.randn(N, C, h, w, generator=gen) * 3).to(dev)
    um0 = (torch.rand(N, 1, H, W, generator=gen) > 0.1).float().to(dev)
    um1 = (torch.rand(N, 1, H, W, generator=gen) > 0.1).float().to(dev)
    lam = torch.tensor(np.random.RandomState(0).beta(0.1, 0.1, size=N), dtype=torch.float32).to(dev)
    cfg = ops.ICTConsistencyConfig(loss_fn=a.loss_fn, conf_thresh=TAU, conf_per_pixel=a.conf_per_pixel, align_corners=True)

    def fused_call():
        sc, ctx = ops.ict_consistency_forward(cfg, ls, l0, l1, lam, (H, W), um0=um0, um1=um1, cons_weight=WEIGHT)
        return sc, ops.ict_consistency_backward(ctx, sc)

    torch_call = lambda: torch_leg(ls, l0, l1, lam, um0, um1, a.loss_fn, a.conf_per_pixel)      # noqa: E731
    for _ in range(a.warmup):
        sc, g_f = fused_call()
        closs, rate, g_t = torch_call()
    torch.cuda.synchronize()
    # same inputs: the two legs must have computed the same loss and gradient before their times are compared
    dl = abs(float(sc[0]) - float(closs)) / abs(float(closs))
    dg = float((g_f - g_t).abs().max() / g_t.abs().max())
    print('inputs: {} x {} x {} x {} -> {} x {}, {}{}; rate {:.4f}; loss rel diff {:.2e}, gradient max diff / max {:.2e}'.format(
        N, C, h, w, H, W, a.loss_fn, ' conf_per_pixel' if a.conf_per_pixel else '', float(rate), dl, dg))
    if not (dl < 1e-4 and dg < 1e-3):
        raise SystemExit('ict_loss_bench: fused and torch legs disagree; timings withheld')

    tf, tt = [], []
    for r in range(a.rounds):
        tf.append(timed(fused_call, a.calls))
        tt.append(timed(torch_call, a.calls))
        print('round {}: fused {:.3f} ms   torch {:.3f} ms   (forward + backward)'.format(r, tf[-1], tt[-1]), flush=True)
    nbytes = compulsory_bytes(a.conf_per_pixel)
    res = {'geometry': [N, C, h, w, H, W], 'loss_fn': a.loss_fn, 'conf_per_pixel': bool(a.conf_per_pixel), 'rounds': a.rounds,
           'calls_per_round': a.calls, 'fused_ms_median': float(np.median(tf)), 'fused_ms_min': min(tf), 'fused_ms_max': max(tf),
           'torch_ms_median': float(np.median(tt)), 'torch_ms_min': min(tt), 'torch_ms_max': max(tt),
           'fused_compulsory_bytes': nbytes, 'torch_materialised_bytes_lower_bound': (5 * C + 4) * N * H * W * 4}
    res['spread_ms'] = max(max(tf) - min(tf), max(tt) - min(tt))
    res['fused_faster_by_more_than_spread'] = bool(res['torch_ms_median'] - res['fused_ms_median'] > res['spread_ms']
                                                   and max(tf) < min(tt))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
