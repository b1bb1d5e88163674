"""CowMask on the device: what one batch of masks costs, and what the CowMix command makes of it.

Per-batch generator time, at 10 x 321 x 321 and 4 x 512 x 1024 with sigma in 4:16 (radius 64). Two routes on the same device in the
same run, alternating, by device events:
    hip      ops.cowmask: csrc/cowmask.hip, three launches, fp64 from the f32 noise onward
    library  the same definition through the library: two grouped F.conv2d in fp64 (groups = N, one row / column of taps per sample,
             zero padding), mean / std, a compare. It lives here, not in the package: it is the yardstick.
and against the HBM floor of a generator that reads the noise once and writes the mask once, 8 B per pixel at --hbm_tb_s. Per route
and shape: a warm-up call, then `--rounds` rounds of `--calls` calls; ms per batch as the median over the rounds with the spread
(max - min). The two masks are compared first (pixels that differ are counted; the library route sums in another order).

End-to-end (`--end_to_end`): img/s of train_seg_semisup_cowmask_mt against train_seg_semisup_mask_mt, each command as a process of its
own, synthetic data, `--arch resnet101_deeplab_imagenet --freeze_bn`, the same crop and batch, the img/s line of the LAST epoch of each
log (the first epoch carries the warm-up). Prints one JSON line at the end. There is no threshold on either figure.
    python tools/cowmask_bench.py [--rounds 5] [--calls 50] [--end_to_end] [--e2e_iters 40]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, REPO)
from cutmix_semisup_seg_amd import mask_gen, ops  # noqa: E402

SHAPES = [(10, 321, 321), (4, 512, 1024)]
SIGMA_RANGE = (4.0, 16.0)


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def library_cowmask(noise, taps, factor):
    """noise f32 (N,1,H,W), taps f64 (N,K), factor f64 (N,) on the device -> f32 (N,1,H,W)"""
    n, k = taps.shape
    r = (k - 1) // 2
    x = noise.double().transpose(0, 1)                                         # (1, N, H, W): one group per sample
    x = F.conv2d(x, taps.reshape(n, 1, 1, k), padding=(0, r), groups=n)
    s = F.conv2d(x, taps.reshape(n, 1, k, 1), padding=(r, 0), groups=n)[0]     # (N, H, W)
    flat = s.reshape(n, -1)
    tau = flat.mean(dim=1) + flat.std(dim=1, unbiased=False) * factor
    return (s <= tau[:, None, None]).float()[:, None]


def generator_times(a, dev):
    results = []
    gen = mask_gen.CowMaskGenerator((0.2, 0.8), SIGMA_RANGE)
    for n, h, w in SHAPES:
        p, sigma = gen.generate_scalars(n, rng=np.random.RandomState(n + h))
        taps_np, radius = gen.kernel_table(sigma)
        taps = torch.from_numpy(taps_np).to(dev)
        factor = torch.from_numpy(gen.threshold_factors(p)).to(dev)
        noise = torch.randn((n, 1, h, w), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
        routes = {'hip': lambda: ops.cowmask(noise, taps, factor, out=out)}
        res = {'shape': [n, h, w], 'radius': radius, 'hbm_floor_ms': 8.0 * n * h * w / (a.hbm_tb_s * 1e12) * 1e3}
        got = routes['hip']().clone()
        try:
            lib = library_cowmask(noise, taps, factor)
            res['pixels_differing_from_library'] = int((lib != got).sum())
            routes['library'] = lambda: library_cowmask(noise, taps, factor)
            del lib
        except Exception as e:                                                 # the yardstick is missing, the figure stands
            res['library_error'] = '{}: {}'.format(type(e).__name__, str(e).splitlines()[0] if str(e) else '')
            print('library route not taken:', res['library_error'], flush=True)
        res['share_of_ones'] = [round(float(v), 4) for v in got.mean(dim=(1, 2, 3)).cpu()]
        res['p'] = [round(float(v), 4) for v in p]
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, f in routes.items():                                        # alternating: both see the same machine
                times[k].append(timed_ms(f, a.calls if k == 'hip' else max(1, a.calls // 5)))
            print('{} round {}: {}'.format((n, h, w), r, {k: round(v[-1], 4) for k, v in times.items()}), flush=True)
        for k in routes:
            res[k + '_ms_median'] = float(np.median(times[k]))
            res[k + '_ms_spread'] = max(times[k]) - min(times[k])
        print(res, flush=True)
        results.append(res)
    return results


def end_to_end(a):
    """img/s of the last epoch of each command, each in a process of its own"""
    out = {}
    common = ['--job_desc', 'bench', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', str(a.e2e_batch),
              '--crop_size', a.e2e_crop, '--learning_rate', '3e-5', '--lr_sched', 'poly', '--num_epochs', '3', '--iters_per_epoch',
              str(a.e2e_iters), '--synthetic_val_batches', '1']
    for name in ('train_seg_semisup_mask_mt', 'train_seg_semisup_cowmask_mt', 'train_seg_semisup_mask_mt', 'train_seg_semisup_cowmask_mt'):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.join(REPO, name + '.py')] + common
            proc = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.e2e_timeout)
            if proc.returncode != 0:
                raise SystemExit('{} ended with {}:\n{}'.format(name, proc.returncode, proc.stdout.decode()[-2000:]))
            log = open(os.path.join(tmp, 'results', name, 'log_bench.txt')).read()
        rates = [float(v) for v in re.findall(r'-- ([\d.]+) img/s', log)]
        print(name, 'img/s per epoch', rates, flush=True)
        out.setdefault(name, []).append(rates[-1])
    return {'crop': a.e2e_crop, 'batch': a.e2e_batch, 'iters_per_epoch': a.e2e_iters,
            'img_per_s_last_epoch': out, 'cowmask_over_cutmix': float(np.mean(out['train_seg_semisup_cowmask_mt']) /
                                                                      np.mean(out['train_seg_semisup_mask_mt']))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--hbm_tb_s', type=float, default=8.0, help='peak HBM bandwidth the floor is taken against')
    ap.add_argument('--end_to_end', action='store_true')
    ap.add_argument('--e2e_crop', default='321,321')
    ap.add_argument('--e2e_batch', type=int, default=10)
    ap.add_argument('--e2e_iters', type=int, default=40)
    ap.add_argument('--e2e_timeout', type=int, default=280)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cowmask_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    result = {'rounds': a.rounds, 'calls_per_round': a.calls, 'sigma_range': list(SIGMA_RANGE), 'generator': generator_times(a, dev)}
    if a.end_to_end:
        torch.cuda.synchronize()
        result['end_to_end'] = end_to_end(a)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
