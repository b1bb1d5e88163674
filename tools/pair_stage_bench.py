"""Staging time of the augmentation trainer's unsupervised batch on the data set path: DeviceAugmenter.stage_pair, N = 10 pairs of
321 x 321 bf16 views cut from Pascal-sized pool entries (375 x 500, 500 x 375, 333 x 500 uint8), for the plain crop, the Hung
scale crop with strong colour (the luminance pre-pass runs) and the rotate / scale crop.

  device  device events around `calls` back-to-back stage_pair(drawn=...) calls with the parameters drawn beforehand -- the
          upload of the 2N rows, the luminance pre-pass over the view-1 half, the pivot, the one launch over 2N rows -- per call;
          `rounds` rounds after a warm-up round
  host    host clock around PairGeometry.draw_batch + aug_pairs.pair_rows + the colour draw for ten pairs (draw_pair_params)

With --step_ms (the trainer's milliseconds per iteration in the same session) the shares are printed. One JSON line (also --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cutmix_semisup_seg_amd.aug_pairs import PairGeometry                       # noqa: E402
from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter             # noqa: E402
from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource     # noqa: E402

N, H, W = 10, 321, 321
SIZES = [(375, 500), (500, 375), (333, 500)]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CASES = dict(crop=(dict(), dict()), hung_colour=(dict(scale_hung=True, hflip=True), dict(strong_colour=True)),
             warp=(dict(rot_mag=30.0, max_scale=1.5, hflip=True), dict()))


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), rounds=[float(x) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--step_ms', type=float, default=0.0)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('pair_stage_bench needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, size=SIZES[i % len(SIZES)] + (3,)).astype(np.uint8) for i in range(N)]
    labels = [np.zeros(im.shape[:2], dtype=np.uint8) for im in images]
    pool = ResidentPool(ArraySource(images, labels), range(N), dev)
    ids = list(range(N))
    result = dict(shape='{} pairs, entries {} uint8 -> 2 x {} x 3 x {} x {} bf16'.format(N, SIZES, N, H, W), calls_per_round=args.calls)
    for name, (geo_cfg, aug_cfg) in CASES.items():
        aug = DeviceAugmenter((H, W), MEAN, STD, out_dtype=torch.bfloat16, rng=np.random.RandomState(1),
                              colour_rng=np.random.RandomState(2), **aug_cfg)
        geo = PairGeometry((H, W), rng=np.random.RandomState(3), **geo_cfg)
        sizes = pool.sizes_of(ids)
        host = []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                drawn = aug.draw_pair_params(geo, sizes)
            host.append((time.perf_counter() - t0) / args.calls * 1e3)
        device = []
        for r in range(args.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                aug.stage_pair(pool, ids, None, drawn=drawn)
            e1.record()
            e1.synchronize()
            device.append(e0.elapsed_time(e1) / args.calls)
        result[name] = dict(device_ms_per_call=stats(device[1:]), host_draw_ms_per_ten_pairs=stats(host[1:]))
        print('{}: device {:.3f} ms per call, host draw {:.3f} ms per ten pairs'.format(
            name, result[name]['device_ms_per_call']['median'], result[name]['host_draw_ms_per_ten_pairs']['median']), flush=True)
    if args.step_ms > 0:
        result['step_ms'] = args.step_ms
        for name in CASES:
            result[name]['share_of_step'] = dict(
                device=result[name]['device_ms_per_call']['median'] / args.step_ms,
                host_draw=result[name]['host_draw_ms_per_ten_pairs']['median'] / args.step_ms)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
