"""The fused affine-warp consistency loss (ops.aug_consistency_forward + aug_consistency_backward: csrc/aug_math.hpp,
csrc/aug_loss.hip) at the Pascal configuration's geometry -- logits 10 x 21 x 41 x 41, loss at 321 x 321 --
against the same loss written with torch ops on the device: materialised bilinear upsamples, F.affine_grid, three F.grid_sample
calls, two softmaxes, the masked mean and autograd back to the low-resolution student logits (train_seg_semisup_aug_mt.py:302-398
as the reference runs it). Per-sample warps: rotations within +-30 degrees, scales within 1/1.5 .. 1.5 (seeded).
Both legs run in one process, alternated round by round after warm-up; a leg's time is the host clock around `calls` forward +
backward calls that end in a device synchronise. Prints per-round times, then one JSON line with the medians, the spread (max - min
over the rounds of each leg) and the bytes the fused path must move.
    python tools/aug_loss_bench.py [--rounds 7] [--calls 100] [--warmup 3] [--loss_fn var] [--conf_per_pixel]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cutmix_semisup_seg_amd import ops  # noqa: E402

N, C, h, w, H, W = 10, 21, 41, 41, 321, 321
TAU, WEIGHT = 0.6, 1.0


def compulsory_bytes():
    """what one forward + backward of the fused path has to move through HBM / L2: the two low-resolution logit tensors (read by
    both launches), view 1's validity mask once per launch and view 0's at four taps per pixel (the taps of neighbouring pixels
    share cache lines: counted once per launch), the gradient rows (zero-fill + atomics: write, read, write)"""
    lo = N * C * h * w * 4
    um = N * H * W * 4
    return 2 * 2 * lo + 2 * 2 * um + 3 * lo


def torch_leg(ls, lt, theta, um0, um1, loss_fn, conf_per_pixel):
    """forward + backward with torch ops (var / kld / logits_var; the default confidence mode or the per-pixel mask)"""
    ls = ls.detach().requires_grad_(True)
    up = lambda t: F.interpolate(t, size=(H, W), mode='bilinear', align_corners=True)       # noqa: E731
    Ls, Lt = up(ls), up(lt)
    grid = F.affine_grid(theta, [N, C, H, W], align_corners=True)
    mask = F.grid_sample(um0, grid, align_corners=True) * um1
    pt = F.grid_sample(F.softmax(Lt, dim=1), grid, align_corners=True)
    cm = (pt.max(dim=1)[0] >= TAU).float()[:, None, :, :]
    rate = cm.mean()
    mask = mask * (cm if conf_per_pixel else rate)
    if loss_fn == 'var':
        d = F.softmax(Ls, dim=1) - pt
        pix = (d * d).sum(dim=1, keepdim=True)
    elif loss_fn == 'kld':
        pix = F.kl_div(F.log_softmax(Ls, dim=1), pt, reduction='none').sum(dim=1, keepdim=True)
    else:
        d = Ls - F.grid_sample(Lt, grid, align_corners=True)
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


def draw_thetas(seed=0):
    """per-sample rotation within +-30 degrees and zoom within 1/1.5 .. 1.5 (log-uniform) about the centre, normalised coordinates"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(N):
        r = math.radians(rng.uniform(-30.0, 30.0))
        s = math.exp(rng.uniform(-math.log(1.5), math.log(1.5)))
        out.append([[math.cos(r) * s, -math.sin(r) * s, 0.0], [math.sin(r) * s, math.cos(r) * s, 0.0]])
    return np.array(out, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--loss_fn', choices=['var', 'kld', 'logits_var'], default='var')
    ap.add_argument('--conf_per_pixel', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('aug_loss_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    ls = (torch.randn(N, C, h, w, generator=gen) * 2).to(dev)
    lt = (torch.randn(N, C, h, w, generator=gen) * 3).to(dev)
    um0 = (torch.rand(N, 1, H, W, generator=gen) > 0.1).float().to(dev)
    um1 = (torch.rand(N, 1, H, W, generator=gen) > 0.1).float().to(dev)
    theta = torch.from_numpy(draw_thetas()).to(dev)
    cfg = ops.AugConsistencyConfig(loss_fn=a.loss_fn, conf_thresh=TAU, conf_per_pixel=a.conf_per_pixel, align_corners=True)

    def fused_call():
        sc, ctx = ops.aug_consistency_forward(cfg, ls, lt, theta, (H, W), um0=um0, um1=um1, cons_weight=WEIGHT)
        return sc, ops.aug_consistency_backward(ctx, sc)

    torch_call = lambda: torch_leg(ls, lt, theta, um0, um1, a.loss_fn, a.conf_per_pixel)      # noqa: E731
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
        raise SystemExit('aug_loss_bench: fused and torch legs disagree; timings withheld')

    tf, tt = [], []
    for r in range(a.rounds):
        tf.append(timed(fused_call, a.calls))
        tt.append(timed(torch_call, a.calls))
        print('round {}: fused {:.3f} ms   torch {:.3f} ms   (forward + backward)'.format(r, tf[-1], tt[-1]), flush=True)
    res = {'geometry': [N, C, h, w, H, W], 'loss_fn': a.loss_fn, 'conf_per_pixel': bool(a.conf_per_pixel), 'rounds': a.rounds,
           'calls_per_round': a.calls, 'fused_ms_median': float(np.median(tf)), 'fused_ms_min': min(tf), 'fused_ms_max': max(tf),
           'torch_ms_median': float(np.median(tt)), 'torch_ms_min': min(tt), 'torch_ms_max': max(tt),
           'fused_compulsory_bytes': compulsory_bytes(), 'torch_materialised_bytes_lower_bound': (6 * C + 5) * N * H * W * 4}
    res['spread_ms'] = max(max(tf) - min(tf), max(tt) - min(tt))
    res['fused_faster_by_more_than_spread'] = bool(res['torch_ms_median'] - res['fused_ms_median'] > res['spread_ms']
                                                   and max(tf) < min(tt))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
