"""Surface distances (HD, HD95, ASSD) on the device: what one batch costs.

Per-batch time of ops.surface_distances (csrc/surface.hip: mark, rows, column walk, partial sums, four select passes) at
10 x 321 x 321 (C = 21), 4 x 512 x 1024 (C = 19) and 1 x 1024 x 2048 (C = 19), by device events: a warm-up call, then `--rounds` rounds
of `--calls` calls; ms per batch as the median over the rounds with the smallest and largest round. The maps are blobs (the argmax of
upsampled noise) with a void frame and a void block in the truth, once `fine` (a noise sample every 24 pixels), once `coarse` (every
200 pixels: surfaces hundreds of pixels apart), and once `lone`: the coarse maps with one class that the truth holds as a single pixel
in a corner and the prediction as a single pixel in the opposite one, so that two column walks run as long as a walk can.

Next to it, clearly not the same kind of number: `scipy_host_s`, the time of the same `stats` from a host restatement with scipy
(binary_erosion with the cross, distance_transform_edt with indices, a sort), run once per shape and kind on the CPU of this machine.
It lives here, not in the package: it is the yardstick, and the package does not import scipy. `integers_differing_from_scipy` must be
0, and the tool ends with an error when it is not. `workspace_mib` is what cms_surface_workspace_bytes asks for; `floor_ms` the time of
reading the two uint8 maps once at 8 TB/s. Prints one JSON line at the end. There is no threshold on any time.
`--eval_batch` adds `eval_forward_ms`: the forward pass of a DeepLab v2 ResNet-101 (random weights, bf16, evaluation mode) on a batch
of the same shape plus the fused upsample / argmax / confusion launch -- what an evaluation batch costs without this call -- and
`share_of_eval_batch` = hip_ms_median / (eval_forward_ms + hip_ms_median).
`--only 2:coarse` measures one shape (by its index) and kind of map alone, as a kernel trace wants it.
    python tools/surface_bench.py [--rounds 5] [--calls 20] [--no_host] [--eval_batch] [--only INDEX:KIND]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, REPO)
from cutmix_semisup_seg_amd import _lib, ops  # noqa: E402

# (N, H, W, C): Pascal VOC crops, Cityscapes at half size, Cityscapes at full size
SHAPES = [(10, 321, 321, 21), (4, 512, 1024, 19), (1, 1024, 2048, 19)]
HBM_BYTES_PER_S = 8e12
IGNORE = 255
GRAIN = {'fine': 24, 'coarse': 200, 'lone': 200}


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def blob_map(n, h, w, c, seed, dev, grain):
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randn((n, c, h // grain + 2, w // grain + 2), generator=g, device=dev)
    return F.interpolate(z, size=(h, w), mode='bilinear', align_corners=False).argmax(dim=1).to(torch.uint8)


def make_maps(n, h, w, c, dev, kind):
    grain = GRAIN[kind]
    k = c - 1 if kind == 'lone' else c                                       # the last class is kept for the two lone pixels
    truth, pred = blob_map(n, h, w, k, 1, dev, grain), blob_map(n, h, w, k, 2, dev, grain)
    pred = torch.where(blob_map(n, h, w, 4, 3, dev, grain) == 0, pred, truth)  # a prediction that is mostly right
    truth[:, :3], truth[:, -5:], truth[:, :, :4], truth[:, :, -2:] = IGNORE, IGNORE, IGNORE, IGNORE
    truth[:, h // 3:h // 3 + 17, w // 2:w // 2 + 29] = IGNORE
    if kind == 'lone':
        truth[:, 3, 4] = c - 1
        pred[:, h - 6, w - 3] = c - 1
    return truth.contiguous(), pred.contiguous()


def scipy_stats(truth, pred, c):
    """the (N, C, 6) int64 `stats` of ops.surface_distances, restated with scipy on the host"""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    n = truth.shape[0]
    stats = np.full((n, c, 6), -1, dtype=np.int64)

    def d2(src, dst):
        iy, ix = ndimage.distance_transform_edt(~dst, return_distances=False, return_indices=True)
        yy, xx = np.nonzero(src)
        return (yy.astype(np.int64) - iy[yy, xx]) ** 2 + (xx.astype(np.int64) - ix[yy, xx]) ** 2
    for i in range(n):
        t = truth[i]
        p = np.where(t == IGNORE, IGNORE, pred[i])
        for cl in range(c):
            border = []
            for m in (p == cl, t == cl):
                border.append(m & ~ndimage.binary_erosion(m, cross, border_value=0) if m.any() else m)
            stats[i, cl, 0], stats[i, cl, 1] = border[0].sum(), border[1].sum()
            if border[0].any() and border[1].any():
                a, b = d2(border[0], border[1]), d2(border[1], border[0])
                pooled = np.sort(np.concatenate([a, b]))
                lo = 19 * (len(pooled) - 1) // 20
                stats[i, cl, 2:] = a.max(), b.max(), pooled[lo], pooled[min(lo + 1, len(pooled) - 1)]
    return stats


def eval_forward_ms(n, h, w, c, dev, calls):
    """ms per evaluation batch without the surface distances: DeepLab v2 ResNet-101 forward and the fused argmax / confusion launch"""
    from cutmix_semisup_seg_amd.architectures import deeplab2
    net = deeplab2.resnet101_deeplab_imagenet(num_classes=c, pretrained=False).to(dev)
    net.compute_dtype = torch.bfloat16
    for p in net.parameters():
        p.requires_grad = False
    net.eval()
    x = torch.randn((n, 3, h, w), device=dev).to(torch.bfloat16)
    labels = torch.zeros((n, 1, h, w), dtype=torch.uint8, device=dev)
    cm = torch.zeros((c, c), dtype=torch.int64, device=dev)

    def batch():
        with torch.no_grad():
            ops.argmax_confusion(net.forward_lowres(x), labels, c, (h, w), ignore_index=255, align_corners=True, cm=cm)
    batch()
    return float(np.median([timed_ms(batch, calls) for _ in range(3)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--no_host', action='store_true', help='skip the scipy restatement (and the comparison with it)')
    ap.add_argument('--eval_batch', action='store_true', help='also time the forward pass of an evaluation batch of the shape')
    ap.add_argument('--only', type=str, default=None, help='INDEX:KIND, e.g. 2:coarse')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('surface_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    results = []
    todo = [s + (k,) for s in SHAPES for k in GRAIN]
    if a.only is not None:
        index, kind = a.only.split(':')
        todo = [SHAPES[int(index)] + (kind,)]
    for n, h, w, c, kind in todo:
        truth, pred = make_maps(n, h, w, c, dev, kind)
        stats, sums, _ = ops.surface_distances(truth, pred, c)
        torch.cuda.synchronize()
        st = stats.cpu().numpy()
        scored = (st[..., 0] > 0) & (st[..., 1] > 0)
        res = {'shape': [n, h, w], 'maps': kind, 'classes': c, 'pairs_scored': int(scored.sum()),
               'surface_pixels': int(st[..., :2].sum()), 'max_d2': int(st[..., 2:4].max()),
               'workspace_mib': _lib.fn['cms_surface_workspace_bytes'](n, h, w, c) / 2.0 ** 20,
               'floor_ms': 2.0 * n * h * w / HBM_BYTES_PER_S * 1e3}
        if not a.no_host:
            t_host, p_host = truth.cpu().numpy(), pred.cpu().numpy()
            t0 = time.perf_counter()
            ref = scipy_stats(t_host, p_host, c)
            res['scipy_host_s'] = time.perf_counter() - t0
            res['integers_differing_from_scipy'] = int((ref != st).sum())
        times = [timed_ms(lambda: ops.surface_distances(truth, pred, c), a.calls) for _ in range(a.rounds)]
        res['hip_ms_median'], res['hip_ms_min'], res['hip_ms_max'] = float(np.median(times)), min(times), max(times)
        res['share_of_floor'] = res['floor_ms'] / res['hip_ms_median']
        if a.eval_batch:
            res['eval_forward_ms'] = eval_forward_ms(n, h, w, c, dev, max(1, a.calls // 4))
            res['share_of_eval_batch'] = res['hip_ms_median'] / (res['eval_forward_ms'] + res['hip_ms_median'])
        print(res, flush=True)
        results.append(res)
    print(json.dumps({'rounds': a.rounds, 'calls_per_round': a.calls, 'surface': results}))
    if any(r.get('integers_differing_from_scipy') for r in results):
        raise SystemExit('surface_bench: the kernel path and the scipy restatement differ')


if __name__ == '__main__':
    main()
