"""
Time the CRF refinement (ops.crf_refine, csrc/crf.hip) against the same definition written in torch operations on the same device:
F.interpolate + softmax for the unary term, then per iteration (2R+1)^2 - 1 shifted views of the padded class probabilities, each
weighted by its pair weight, summed, divided by the neighbour count; softmax; argmax.

    python tools/crf_bench.py [--rounds 5] [--calls 50] [--torch_calls 5]

Device events around `--calls` back-to-back calls of a leg (`--torch_calls` of the torch leg, which is the slower by far); one
warm-up, then `--rounds` rounds in which the legs alternate in one process; medians over the rounds, per call. The labels of the two
legs are compared before anything is timed (they may differ where two classes' Q are within fp32 rounding of each other; the count
is printed). Prints one JSON line per shape: milliseconds per call of both legs, the peak memory each leg allocates beyond its
inputs, and for the mean-field launch its time per iteration -- (time at T iterations - time at 1) / (T - 1) -- against two floors
worked out from its own counts: the LDS floor (per pixel and iteration (2R+1)^2 - 1 neighbours x (chunk + 1) four-byte reads at
128 B per clock and CU) and the VALU floor (neighbours x chunk fused multiply-adds at 128 per clock and CU), 256 CUs at 2.4 GHz.
No threshold: nothing exists to regress against.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (N, C, (h, w), (H, W), align_corners): Pascal VOC at 321 x 321 from 41 x 41 logits, Cityscapes at 512 x 1024 from 65 x 129
SHAPES = {
    'pascal': (10, 21, (41, 41), (321, 321), True),
    'cityscapes': (4, 19, (65, 129), (512, 1024), True),
}
CUS, CLOCK_HZ, LDS_BYTES_PER_CLK_CU, FMA_PER_CLK_CU = 256, 2.4e9, 128, 128


def torch_crf(logits, rgb, size, align, prm):
    """the definition with every rectangle the whole canvas -> (labels, labels that differ from the unary ones)"""
    R, S, T = prm.radius, prm.dilation, prm.iters
    p = torch.softmax(F.interpolate(logits, size=size, mode='bilinear', align_corners=align), dim=1)
    logp = torch.log(p.clamp_min(torch.finfo(torch.float32).tiny))
    pad = R * S
    img = F.pad(rgb.float(), (pad, pad, pad, pad))
    ones = F.pad(torch.ones_like(p[:, :1]), (pad, pad, pad, pad))
    H, W = size
    shifts = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dy, dx) != (0, 0)]
    view = lambda t, dy, dx: t[:, :, pad + S * dy:pad + S * dy + H, pad + S * dx:pad + S * dx + W]
    count = sum(view(ones, dy, dx) for dy, dx in shifts)
    weights = []
    for dy, dx in shifts:
        d2 = float(S * S * (dy * dy + dx * dx))
        di = ((rgb.float() - view(img, dy, dx)) ** 2).sum(dim=1, keepdim=True)
        weights.append((prm.bi_w * torch.exp(-d2 / (2 * prm.bi_xy ** 2) - di / (2 * prm.bi_rgb ** 2))
                        + prm.pos_w * float(np.exp(-d2 / (2 * prm.pos_xy ** 2)))) * view(ones, dy, dx))
    q = p
    for _ in range(T):
        qp = F.pad(q, (pad, pad, pad, pad))
        msg = torch.zeros_like(q)
        for (dy, dx), wq in zip(shifts, weights):
            msg += wq * view(qp, dy, dx)
        q = torch.softmax(logp + msg / count.clamp_min(1.0), dim=1)
    return q.argmax(dim=1), p.argmax(dim=1)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--torch_calls', type=int, default=5)
    ap.add_argument('--shapes', type=str, default=','.join(SHAPES))
    args = ap.parse_args()
    from cutmix_semisup_seg_amd import ops
    from cutmix_semisup_seg_amd.crf import CRFParams
    dev = torch.device('cuda', 0)
    prm = CRFParams()
    one = CRFParams(iters=1)
    for name in args.shapes.split(','):
        n, c, (h, w), size, align = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(0)
        logits = torch.randn(n, c, h, w, generator=g, device=dev) * 3.0
        # piecewise constant image: 8 x 8 blocks of random colour plus noise
        blocks = torch.rand(n, 3, (size[0] + 7) // 8, (size[1] + 7) // 8, generator=g, device=dev) * 255.0
        rgb = blocks.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :size[0], :size[1]]
        rgb = (rgb + (torch.rand(rgb.shape, generator=g, device=dev) - 0.5) * 15.0).round().clamp(0, 255).to(torch.uint8).contiguous()
        rects = np.array([[0, 0, size[0], size[1]]] * n, dtype=np.int32)
        fused = lambda p=prm: ops.crf_refine([logits], [False], rgb, rects, c, size, p, align_corners=align)
        plain = lambda: torch_crf(logits, rgb, size, align, prm)
        (_, pf, _, stats), fused_peak = peak_of(fused)                    # the warm-up, the comparison and the peaks
        (pt, ut), torch_peak = peak_of(plain)
        fused(one)
        differ = int((pf.long() != pt).sum())
        changed_torch = int((pt != ut).sum())
        times = {'fused': [], 'fused_one_iter': [], 'torch': []}
        for _ in range(args.rounds):
            times['fused'].append(timed(fused, args.calls))
            times['torch'].append(timed(plain, args.torch_calls))
            times['fused_one_iter'].append(timed(lambda: fused(one), args.calls))
        out = dict(shape=name, n=n, c=c, size=size, params=prm.as_dict(), labels_that_differ=differ,
                   labels_changed_fused=int(stats[1]), labels_changed_torch=changed_torch, pixels=int(stats[0]),
                   fused_peak_bytes=int(fused_peak), torch_peak_bytes=int(torch_peak))
        med = {}
        for route, ts in times.items():
            ts = sorted(ts)
            med[route] = ts[len(ts) // 2]
            out[route + '_ms_median'] = round(ts[len(ts) // 2], 4)
            out[route + '_ms_min'] = round(ts[0], 4)
            out[route + '_ms_max'] = round(ts[-1], 4)
        per_iter = (med['fused'] - med['fused_one_iter']) / (prm.iters - 1) * 1e-3
        chunk = next(v for v in (4, 8, 16, 24, 32) if min(c, 32) <= v)
        taps = (2 * prm.radius + 1) ** 2 - 1
        pixels = n * size[0] * size[1]
        passes = -(-c // 32)
        lds_floor = pixels * taps * (chunk + 1) * passes * 4 / (CUS * LDS_BYTES_PER_CLK_CU * CLOCK_HZ)
        valu_floor = pixels * taps * chunk * passes / (CUS * FMA_PER_CLK_CU * CLOCK_HZ)
        out.update(meanfield_ms_per_iter=round(per_iter * 1e3, 4), lds_floor_ms=round(lds_floor * 1e3, 4),
                   valu_floor_ms=round(valu_floor * 1e3, 4), share_of_lds_floor=round(lds_floor / per_iter, 3),
                   share_of_valu_floor=round(valu_floor / per_iter, 3))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
