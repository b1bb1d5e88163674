"""The four neighbouring-patch distance maps (int64 squared distances: left, right, up, down) of one pool entry at the Cityscapes
geometry of the reference's programs, a synthetic 512 x 1024 image, for p = 15, 31 and 225. Two routes on the same device in the
same run, alternating, by device events:
    hip     patch_dist.neighbour_sqr_distance_maps: csrc/patchdist.hip, squared neighbour differences and two running-sum passes
    torch   the test-side restatement (tests/_neighbour_dist_refs.py torch_neighbour_d2): gather-pad and an int64 torch.cumsum
            summed-area table per direction. It is the yardstick, not the code under test.
Per route and p: a warm-up call, then `--rounds` rounds of `--calls` calls; ms per image as the median over the rounds with the
spread (max - min), and the launches per image as the profiler counts them in one further call. The two results are compared for
equality first. Prints one JSON line at the end. There is no threshold: nothing exists to regress against.
    python tools/neighbour_dist_bench.py [--rounds 5] [--calls 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from cutmix_semisup_seg_amd import patch_dist as pd  # noqa: E402
from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource  # noqa: E402
import _neighbour_dist_refs as R  # noqa: E402

H, W, SIZES = 512, 1024, (15, 31, 225)


def synthetic(rng):
    """a smooth image with noise on top and one flat region: what a street scene looks like to these kernels"""
    lo = rng.randint(0, 256, size=(H // 16 + 1, W // 16 + 1, 3))
    img = lo.repeat(16, 0).repeat(16, 1)[:H, :W] + rng.randint(-8, 9, size=(H, W, 3))
    img[H // 2:, W // 2:] = 90
    return np.clip(img, 0, 255).astype(np.uint8)


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def launches(fn):
    """device kernels and memory operations of one call, as the profiler sees them"""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('neighbour_dist_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    image = synthetic(np.random.RandomState(0))
    pool = ResidentPool(ArraySource([image]), [0], dev, with_labels=False)
    image_dev = torch.from_numpy(image).to(dev)
    results = []
    for p in SIZES:
        routes = {'hip': lambda: pd.neighbour_sqr_distance_maps(pool, 0, (p, p)), 'torch': lambda: R.torch_neighbour_d2(image_dev, (p, p))}
        got = {k: f() for k, f in routes.items()}                         # warm-up, and the check that both compute the same
        equal = bool(torch.equal(got['hip'], got['torch']))
        zeros = int((got['hip'] == 0).sum())
        del got
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, f in routes.items():                                   # alternating: both see the same machine
                times[k].append(timed_ms(f, a.calls))
            print('p {:3d} round {}: hip {:.4f} ms   torch {:.4f} ms   per image'.format(p, r, times['hip'][-1], times['torch'][-1]),
                  flush=True)
        res = {'p': p, 'equal': equal, 'exact_zeros': zeros}
        for k in routes:
            res[k + '_ms_median'] = float(np.median(times[k]))
            res[k + '_ms_spread'] = max(times[k]) - min(times[k])
        print('p {:3d}: {}'.format(p, res), flush=True)
        results.append(res)
    # the launch counts last, in calls of their own: the profiler slows the host, so nothing above is timed under it
    for res in results:
        p = res['p']
        for k, f in (('hip', lambda: pd.neighbour_sqr_distance_maps(pool, 0, (p, p))),
                     ('torch', lambda: R.torch_neighbour_d2(image_dev, (p, p)))):
            try:
                res[k + '_launches'] = launches(f)
            except Exception as e:                                        # a side figure: the times stand without it
                res[k + '_launches'] = None
                print('launch count of {} not taken: {}'.format(k, e))
    print(json.dumps({'geometry': [H, W], 'rounds': a.rounds, 'calls_per_round': a.calls, 'results': results}))


if __name__ == '__main__':
    main()
