"""
Time the fused test-time-augmentation vote (ops.tta_vote, csrc/tta.hip) against the same vote written in torch operations on the
same device: per view F.interpolate to the output size, flip, softmax, sum; then argmax.

    python tools/tta_bench.py [--rounds 5]

Device events around each route; one warm-up, then `--rounds` rounds in which the two routes alternate in one process. The
predictions of the two routes are compared before anything is timed (they may differ where the summed probabilities of two classes
are within fp32 rounding of each other; the count is printed). Prints one JSON line per shape: median and spread of both routes
in milliseconds, and the bytes the torch route materialises (K upsampled logit tensors, K probability tensors, and the running
sum: fp32 (N, C, H, W) each). No threshold: nothing exists to regress against.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (N, C, (H, W), view sizes, align_corners): Cityscapes at 512 x 1024 with six scales and their mirror images, views from the
# 65 x 129 family; Pascal VOC at 321 x 321 from 41 x 41 views
SHAPES = {
    'cityscapes_k12': (4, 19, (512, 1024), [(33, 65), (33, 65), (49, 97), (49, 97), (65, 129), (65, 129), (81, 161), (81, 161),
                                            (97, 193), (97, 193), (113, 225), (113, 225)], True),
    'pascal_k1': (10, 21, (321, 321), [(41, 41)], True),
    'pascal_k2': (10, 21, (321, 321), [(41, 41), (41, 41)], True),
}


def torch_vote(logits, flips, size, align):
    score = None
    for lg, f in zip(logits, flips):
        up = F.interpolate(lg, size=size, mode='bilinear', align_corners=align)
        if f:
            up = up.flip(-1)
        if len(logits) == 1:
            score = up
            break
        p = torch.softmax(up, dim=1)
        score = p if score is None else score + p
    return score.argmax(dim=1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    from cutmix_semisup_seg_amd import ops
    dev = torch.device('cuda', 0)
    for name, (n, c, size, views, align) in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(0)
        logits = [torch.randn(n, c, h, w, generator=g, device=dev) * 3.0 for h, w in views]
        flips = [bool(i % 2) for i in range(len(views))]
        fused = lambda: ops.tta_vote(logits, flips, c, size, align_corners=align, want_pred=True)[1]
        plain = lambda: torch_vote(logits, flips, size, align)
        pf, pt = fused(), plain()                                       # the warm-up, and the comparison
        differ = int((pf.long() != pt).sum())
        assert differ <= pf.numel() // 1000, 'the two routes disagree on {} of {} pixels'.format(differ, pf.numel())
        times = {'fused': [], 'torch': []}
        for _ in range(args.rounds):
            times['fused'].append(timed(fused))
            times['torch'].append(timed(plain))
        k = len(views)
        nbytes = (2 * k + 1 if k > 1 else 1) * n * c * size[0] * size[1] * 4
        out = dict(shape=name, n=n, c=c, size=size, k=k, pixels_that_differ=differ, torch_bytes_materialised=nbytes)
        for route, ts in times.items():
            ts = sorted(ts)
            out[route + '_ms_median'] = round(ts[len(ts) // 2], 4)
            out[route + '_ms_min'] = round(ts[0], 4)
            out[route + '_ms_max'] = round(ts[-1], 4)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
