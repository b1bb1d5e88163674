"""
Time sliding-window evaluation around the network (ops.window_crop + ops.window_vote, csrc/window.hip) against the same definition
(include/cutmixseg.h) written in torch operations on the same device: per view ops.tta_resize and slicing into a window batch; then
per view F.interpolate of the window logits to the window, softmax, accumulation of the windows into a view canvas by slicing beside
a count map, the division, the read of the view at every canvas pixel (a view that one window holds is interpolated straight to the
canvas, as the definition has it); the views summed, argmax, and a bincount against the labels.

    python tools/window_bench.py [--rounds 5] [--calls 20]

The network is not part of either route: the window logits are random tensors of the size a DeepLab head gives ((e - 1) / 8 + 1).
Device events around `--calls` calls of a route; one warm-up, then `--rounds` rounds in which the two routes alternate in one
process; the medians over the rounds are reported per call. The labels of the two routes are compared before anything is timed
(they may differ where the scores of two classes are within fp32 rounding of each other; the count is printed), and each route's
peak allocation above what is resident before it is measured in a call of its own. Prints one JSON line per shape. No threshold:
nothing exists to regress against.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIX = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
# name -> (N, C, canvas, window, scales, flip)
SHAPES = {
    'cityscapes_half_4x19_w256x512': (4, 19, (512, 1024), (256, 512), (1.0,), False),
    'cityscapes_full_1x19_w512x1024': (1, 19, (1024, 2048), (512, 1024), (1.0,), False),
    'cityscapes_full_1x19_w512x1024_six_scales_flip': (1, 19, (1024, 2048), (512, 1024), SIX, True),
}


def view_coord(canvas, view, dev):
    y = torch.arange(canvas, device=dev, dtype=torch.int64)
    return torch.clamp(((2 * y + 1) * view) // (2 * canvas), max=view - 1)


def torch_crop(image, view, flip, windows):
    from cutmix_semisup_seg_amd import ops
    canvas = tuple(image.shape[2:])
    full = image if (view == canvas and not flip) else ops.tta_resize(image, view, flip=flip)
    (eh, ew), (ys, xs) = windows.extent(view), windows.origins(view)
    return torch.stack([full[:, :, y1:y1 + eh, x1:x1 + ew] for y1 in ys for x1 in xs], dim=1).flatten(0, 1)


def torch_stitch(logits, flips, views, windows, canvas, align, labels, c):
    H, W = canvas
    dev = logits[0].device
    score = None
    for l, flip, view in zip(logits, flips, views):
        (gy, gx), (eh, ew), (ys, xs) = windows.grid(view), windows.extent(view), windows.origins(view)
        n = l.shape[0] // (gy * gx)
        if gy * gx == 1:
            # one window holds the view: it is read as the vote over whole views reads it, straight at the canvas' size
            up = F.interpolate(l, size=canvas, mode='bilinear', align_corners=align)
            part = (up.flip(-1) if flip else up).softmax(1)
            score = part if score is None else score + part
            continue
        p = F.interpolate(l, size=(eh, ew), mode='bilinear', align_corners=align).softmax(1).view(n, gy, gx, c, eh, ew)
        acc = torch.zeros((n, c) + tuple(view), device=dev)
        cnt = torch.zeros(tuple(view), device=dev)
        for j, y1 in enumerate(ys):
            for i, x1 in enumerate(xs):
                acc[:, :, y1:y1 + eh, x1:x1 + ew] += p[:, j, i]
                cnt[y1:y1 + eh, x1:x1 + ew] += 1
        acc /= cnt
        if view == canvas and not flip:
            part = acc
        else:
            ry, rx = view_coord(H, view[0], dev), view_coord(W, view[1], dev)
            if flip:
                rx = view[1] - 1 - rx
            part = acc[:, :, ry[:, None], rx[None, :]]
        score = part if score is None else score + part
    pred = score.argmax(1)
    keep = labels != 255
    cm = torch.bincount(labels[keep].long() * c + pred[keep], minlength=c * c).view(c, c)
    return pred, cm


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
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    from cutmix_semisup_seg_amd import ops
    from cutmix_semisup_seg_amd.tta import TTA, Windows
    dev = torch.device('cuda', 0)
    for name, (n, c, canvas, window, scales, flip) in SHAPES.items():
        tta, windows = TTA(scales, flip), Windows(window)
        g = torch.Generator(device=dev).manual_seed(0)
        image = torch.randn((n, 3) + canvas, generator=g, device=dev).bfloat16()
        labels = torch.randint(0, c, (n,) + canvas, generator=g, device=dev).to(torch.uint8)
        labels[:, :8] = 255
        views = [tta.view_size(canvas, (1, 1), s) for s, _ in tta.views()]
        flips = [f for _, f in tta.views()]
        logits = []
        for view in views:
            eh, ew = windows.extent(view)
            logits.append(torch.randn(n * windows.count(view), c, (eh - 1) // 8 + 1, (ew - 1) // 8 + 1, generator=g, device=dev) * 3.0)

        def fused():
            for view, f in zip(views, flips):
                ops.window_crop(image, view, f, windows.window, windows.stride)
            cm, pred = ops.window_vote(logits, flips, views, windows.window, windows.stride, c, canvas, labels=labels,
                                       align_corners=True, want_pred=True)
            return pred, cm

        def plain():
            for view, f in zip(views, flips):
                torch_crop(image, view, f, windows)
            return torch_stitch(logits, flips, views, windows, canvas, True, labels, c)

        (pf, cf), (pt, ct) = fused(), plain()                             # the warm-up, and the comparison
        differ = int((pf.long() != pt).sum())
        assert differ <= pf.numel() // 1000, 'the two routes disagree on {} of {} pixels'.format(differ, pf.numel())
        assert int(cf.sum()) == int(ct.sum())
        del pf, cf, pt, ct
        peaks = {'fused': peak_of(fused), 'torch': peak_of(plain)}
        times = {'fused': [], 'torch': []}
        for _ in range(args.rounds):
            times['fused'].append(timed(fused, args.calls))
            times['torch'].append(timed(plain, args.calls))
        out = dict(shape=name, n=n, c=c, canvas=canvas, window=windows.window, stride=windows.stride, views=len(views),
                   windows=sum(n * windows.count(v) for v in views), labels_that_differ=differ, pixels=n * canvas[0] * canvas[1])
        for route, ts in times.items():
            ts = sorted(ts)
            out[route + '_ms_median'] = round(ts[len(ts) // 2], 4)
            out[route + '_ms_min'] = round(ts[0], 4)
            out[route + '_ms_max'] = round(ts[-1], 4)
            out[route + '_peak_mib'] = round(peaks[route] / 2.0 ** 20, 1)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
