"""Boundary IoU / trimap IoU counts on the device: what one batch costs.

Per-batch time of ops.boundary_confusion (csrc/boundary.hip: a row pass, a column pass, a counting pass) at one width, at
10 x 321 x 321 (C = 21, d = 9), 4 x 512 x 1024 (C = 19, d = 23) and 1 x 1024 x 2048 (C = 19, d = 46) -- the widths are 2 % of each
shape's diagonal, Boundary IoU's default -- against one yardstick on the same device in the same run, alternating, by device events:
    torch  the same two matrices in torch operations: the class masks as an (N, C, H, W) half tensor, the band of a mask as the mask
           and the max_pool2d of window 2d + 1 of its complement (outside the array counts as complement; the square window as a
           column pool after a row pool), the band labels by masks, `bincount`. It lives here, not in the package: it is the
           yardstick. Its peak memory (torch.cuda.max_memory_allocated over one call, above what was allocated before it) is recorded.
The maps are blobs (the argmax of upsampled noise) with a void frame and a void block in the truth, once `fine` (a noise sample
every 24 pixels: regions narrower than most bands) and once `coarse` (every 200 pixels: regions hundreds of pixels wide, where the
column walk of an interior pixel runs its longest). Per route, shape and kind of map: a warm-up call,
then `--rounds` rounds of `--calls` calls (a fifth of them for torch); ms per batch as the median over the rounds with the smallest and
largest round. The matrices of the two routes are compared first: `entries_differing_from_torch` must be 0, and the tool ends with an
error when it is not. `share_of_floor` is the time of reading the two uint8 maps once at 8 TB/s over the kernel path's time. Prints one
JSON line at the end. There is no threshold on any time.
    python tools/boundary_bench.py [--rounds 5] [--calls 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, REPO)
from cutmix_semisup_seg_amd import ops  # noqa: E402

# (N, H, W, C, d): Pascal VOC crops, Cityscapes at half size, Cityscapes at full size
SHAPES = [(10, 321, 321, 21, 9), (4, 512, 1024, 19, 23), (1, 1024, 2048, 19, 46)]
HBM_BYTES_PER_S = 8e12
IGNORE = 255


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


GRAIN = {'fine': 24, 'coarse': 200}


def blob_map(n, h, w, c, seed, dev, grain):
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randn((n, c, h // grain + 2, w // grain + 2), generator=g, device=dev)
    return F.interpolate(z, size=(h, w), mode='bilinear', align_corners=False).argmax(dim=1).to(torch.uint8)


def make_maps(n, h, w, c, dev, grain):
    truth, pred = blob_map(n, h, w, c, 1, dev, grain), blob_map(n, h, w, c, 2, dev, grain)
    pred = torch.where(blob_map(n, h, w, 4, 3, dev, grain) == 0, pred, truth)  # a prediction that is mostly right
    truth[:, :3], truth[:, -5:], truth[:, :, :4], truth[:, :, -2:] = IGNORE, IGNORE, IGNORE, IGNORE
    truth[:, h // 3:h // 3 + 17, w // 2:w // 2 + 29] = IGNORE
    return truth.contiguous(), pred.contiguous()


def torch_boundary(truth, pred, c, d):
    """-> bcm (c+1, c+1), tcm (c, c) int64"""
    live = truth != IGNORE
    blanked = torch.where(live, pred, torch.full_like(pred, IGNORE))
    classes = torch.arange(c, device=truth.device, dtype=torch.uint8)[None, :, None, None]

    def band(m):
        inside = (m[:, None] == classes)
        comp = F.pad((~inside).half(), (d, d, d, d), value=1.0)
        near = F.max_pool2d(F.max_pool2d(comp, (2 * d + 1, 1), stride=1), (1, 2 * d + 1), stride=1)
        return (inside & (near > 0)).any(dim=1)
    bt, bp = band(truth), band(blanked)
    counted = live & (truth < c) & (pred < c)
    t, p = truth.long(), pred.long()
    tq = torch.where(bt, t, torch.full_like(t, c))[counted]
    pq = torch.where(bp, p, torch.full_like(p, c))[counted]
    bcm = torch.bincount(tq * (c + 1) + pq, minlength=(c + 1) ** 2).view(c + 1, c + 1)
    sel = counted & bt
    tcm = torch.bincount(t[sel] * c + p[sel], minlength=c * c).view(c, c)
    return bcm, tcm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('boundary_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    results = []
    for n, h, w, c, d, kind in [s + (k,) for s in SHAPES for k in GRAIN]:
        truth, pred = make_maps(n, h, w, c, dev, GRAIN[kind])
        bcm = torch.zeros((1, c + 1, c + 1), dtype=torch.int64, device=dev)
        tcm = torch.zeros((1, c, c), dtype=torch.int64, device=dev)
        routes = {'hip': lambda: ops.boundary_confusion(truth, pred, c, [d], bcm=bcm, tcm=tcm),
                  'torch': lambda: torch_boundary(truth, pred, c, d)}
        got_b, got_t, _ = ops.boundary_confusion(truth, pred, c, [d])
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ref_b, ref_t = routes['torch']()
        torch.cuda.synchronize()
        peak = int(torch.cuda.max_memory_allocated(dev) - base)
        differ = int((ref_b != got_b[0]).sum()) + int((ref_t != got_t[0]).sum())
        floor_ms = 2.0 * n * h * w / HBM_BYTES_PER_S * 1e3
        res = {'shape': [n, h, w], 'maps': kind, 'classes': c, 'width': d, 'entries_differing_from_torch': differ, 'torch_peak_bytes': peak,
               'pixels_counted': int(got_b.sum()), 'pixels_in_truth_band': int(got_t.sum()), 'floor_ms': floor_ms}
        routes['hip']()
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, f in routes.items():                                        # alternating: both see the same machine
                times[k].append(timed_ms(f, a.calls if k != 'torch' else max(1, a.calls // 5)))
            print('{} {} round {}: {}'.format(res['shape'], kind, r, {k: round(v[-1], 4) for k, v in times.items()}), flush=True)
        for k in routes:
            res[k + '_ms_median'] = float(np.median(times[k]))
            res[k + '_ms_min'], res[k + '_ms_max'] = min(times[k]), max(times[k])
        res['share_of_floor'] = floor_ms / res['hip_ms_median']
        res['torch_over_hip'] = res['torch_ms_median'] / res['hip_ms_median']
        print(res, flush=True)
        results.append(res)
    print(json.dumps({'rounds': a.rounds, 'calls_per_round': a.calls, 'boundary': results}))
    if any(r['entries_differing_from_torch'] for r in results):
        raise SystemExit('boundary_bench: the kernel path and the torch formulation differ')


if __name__ == '__main__':
    main()
