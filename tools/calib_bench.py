"""
Time the calibration launch (ops.calibration_accumulate, csrc/calib.hip) against (a) the vote launch it takes the place of
(ops.tta_vote on the same views, labels and confusion matrix: the parent's kernel) and (b) the same integer tables from torch
operations on the same device: per view F.interpolate to the output size, flip, softmax, sum; max, bucketize, index_add.

    python tools/calib_bench.py [--rounds 5] [--calls 50]

Device events around `--calls` back-to-back calls of a route; one warm-up, then `--rounds` rounds in which the routes alternate in one
process; the median round, per call. The tables of the two routes are compared before anything is timed: the count of integers that
differ is printed (a confidence within fp32 rounding of a bin edge, or two classes within rounding of each other, moves a pixel to
another cell; the fixed-point sums differ where expf / logf round otherwise). Prints one JSON line per shape: the three routes in
milliseconds per call, the extra cost over the vote launch, the launch's byte floor (the views' logits and the labels read once, the
prediction written once, at 8 TB/s) and its share of the launch, and the torch route's peak memory. No threshold: nothing exists to
regress against.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12

# name -> (N, C, (H, W), view sizes, align_corners): Pascal VOC at 321 x 321 from 41 x 41 views; Cityscapes at 512 x 1024 with six
# scales and their mirror images, views from the 65 x 129 family
SHAPES = {
    'pascal_k1': (10, 21, (321, 321), [(41, 41)], True),
    'pascal_k2': (10, 21, (321, 321), [(41, 41), (41, 41)], True),
    'cityscapes_k1': (4, 19, (512, 1024), [(65, 129)], True),
    'cityscapes_k12': (4, 19, (512, 1024), [(33, 65), (33, 65), (49, 97), (49, 97), (65, 129), (65, 129), (81, 161), (81, 161),
                                            (97, 193), (97, 193), (113, 225), (113, 225)], True),
}


def torch_tables(logits, flips, labels, size, align, edges, c):
    """the definition of include/cutmixseg.h at T = 1 in torch operations -> (hist (C, nb, 3), scores (3,), cm (C, C)) int64"""
    k = len(logits)
    ups = []
    for lg, f in zip(logits, flips):
        up = F.interpolate(lg, size=size, mode='bilinear', align_corners=align)
        ups.append(up.flip(-1) if f else up)
    lab = labels.long()
    valid = (lab != 255) & (lab < c)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    if k == 1:
        pred = ups[0].argmax(dim=1)
        pbar = torch.softmax(ups[0], dim=1)
        nll = -torch.log_softmax(ups[0], dim=1).gather(1, safe[:, None])[:, 0]
    else:
        pbar = None
        for up in ups:
            p = torch.softmax(up, dim=1)
            pbar = p if pbar is None else pbar + p
        pred = pbar.argmax(dim=1)
        pbar = pbar / k
        nll = -torch.log(pbar.gather(1, safe[:, None])[:, 0].clamp_min(torch.finfo(torch.float32).tiny))
    conf = pbar.gather(1, pred[:, None])[:, 0].clamp_max(1.0)
    onehot = F.one_hot(safe, c).permute(0, 3, 1, 2)
    brier = ((pbar - onehot) ** 2).sum(dim=1)
    nb = len(edges) + 1
    b = torch.bucketize(conf, edges, right=True)
    cell = (pred * nb + b)[valid]
    fx = lambda v, scale, cap: torch.round(v.clamp(0.0, cap).double() * scale).long()
    hist = torch.zeros((c * nb, 3), dtype=torch.int64, device=conf.device)
    hist[:, 0] = torch.bincount(cell, minlength=c * nb)
    hist[:, 1] = torch.bincount(cell[(pred == lab)[valid]], minlength=c * nb)
    hist[:, 2].index_add_(0, cell, fx(conf[valid], 2.0 ** 24, 1.0))
    scores = torch.stack([valid.sum(), fx(brier[valid], 2.0 ** 24, 2.0).sum(), fx(nll[valid], 2.0 ** 20, 88.0).sum()])
    cm = torch.bincount(lab[valid] * c + pred[valid], minlength=c * c).view(c, c)
    return hist.view(c, nb, 3), scores, cm


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    args = ap.parse_args()
    from cutmix_semisup_seg_amd import evaluation, ops
    dev = torch.device('cuda', 0)
    edges_np = evaluation.calibration_edges(15, evaluation.CALIB_DEFAULT_THRESHOLDS)[0]
    edges = torch.from_numpy(edges_np).to(dev)
    temps = np.ones(1, dtype=np.float32)
    for name, (n, c, size, views, align) in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(0)
        logits = [torch.randn(n, c, h, w, generator=g, device=dev) * 3.0 for h, w in views]
        flips = [bool(i % 2) for i in range(len(views))]
        labels = torch.randint(0, c, (n,) + size, generator=g, device=dev).to(torch.uint8)
        labels[torch.rand((n,) + size, generator=g, device=dev) < 0.1] = 255
        nb = len(edges_np) + 1
        hist = torch.zeros((c, nb, 3), dtype=torch.int64, device=dev)
        scores = torch.zeros(3, dtype=torch.int64, device=dev)
        cm = torch.zeros((c, c), dtype=torch.int64, device=dev)
        pred = torch.empty((n,) + size, dtype=torch.uint8, device=dev)
        calib = lambda: ops.calibration_accumulate(logits, flips, c, size, labels, edges_np, temps, hist, scores,
                                                   align_corners=align, cm=cm, pred=pred)
        vote = lambda: ops.tta_vote(logits, flips, c, size, labels=labels, align_corners=align, cm=cm, pred=pred)
        plain = lambda: torch_tables(logits, flips, labels, size, align, edges, c)
        calib()                                                        # the warm-up, and the comparison
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t_hist, t_scores, t_cm = plain()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        differ = int((hist != t_hist).sum() + (scores != t_scores).sum() + (cm != t_cm).sum())
        moved = int((hist[:, :, 0] - t_hist[:, :, 0]).abs().sum()) // 2
        vote()
        times = {'calib': [], 'vote': [], 'torch': []}
        for _ in range(args.rounds):
            times['calib'].append(timed(calib, args.calls))
            times['vote'].append(timed(vote, args.calls))
            times['torch'].append(timed(plain, max(1, args.calls // 10)))
        pixels = n * size[0] * size[1]
        floor_ms = (sum(t.numel() * 4 for t in logits) + 2 * pixels) / HBM_BYTES_PER_S * 1e3
        out = dict(shape=name, n=n, c=c, size=size, k=len(views), bins=nb, integers=int(hist.numel() + scores.numel() + cm.numel()),
                   integers_that_differ=differ, pixels_in_another_cell=moved, torch_peak_bytes=int(peak))
        for route, ts in times.items():
            ts = sorted(ts)
            out[route + '_ms_median'] = round(ts[len(ts) // 2], 4)
            out[route + '_ms_min'] = round(ts[0], 4)
            out[route + '_ms_max'] = round(ts[-1], 4)
        out['extra_over_vote_ms'] = round(out['calib_ms_median'] - out['vote_ms_median'], 4)
        out['byte_floor_ms'] = round(floor_ms, 5)
        out['floor_share_of_launch'] = round(floor_ms / out['calib_ms_median'], 4)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
