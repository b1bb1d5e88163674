"""Class-threshold consistency on the device: what the per-class thresholds and their statistics cost in the loss launch.

Per-batch time of the fused class-threshold launch plus the update launch (ops.consistency_fused with a ClassThresholds, then
ClassThresholds.update(): csrc/cthresh.hip) against the fixed-threshold launch it replaces (ops.consistency_fused as it was:
cms_consistency_fwd_bwd) on identical inputs, at 10 x 21 x 41x41 -> 321x321 and 4 x 19 x 65x129 -> 512x1024, mix mode, a box table,
both validity maps, the `var` loss, alternating in the same run, by device events. Each route includes its finalising launch and the
deferred scaling of the gradient rows, as the step issues them. Beside them the same thresholds and statistics in torch operations:
    torch  F.interpolate of both teacher logit tensors to (N, C, H, W), `where` by the mask, softmax, max / argmax, the compare with
           thr[argmax], and the sums n_valid, sum conf, sum_c q_c, N_pred, N_pass (bincount). It lives here, not in the package: it is
           the yardstick. Its peak memory above what was allocated before it is recorded, and how far its per-class counts lie
           from the kernel's: sum over classes of |N_pass - N_pass| and of |N_pred - N_pred| (differences of COUNTS, not of bit
           maps: two opposite flips within a class cancel; the torch route interpolates in another order).
Per route and shape: a warm-up call, then `--rounds` rounds of `--calls` calls; ms per batch as the median over the rounds with the
smallest and largest round. The yardstick for the added cost is the fixed launch itself, the margin its own min-max spread.

End-to-end (`--end_to_end`): img/s of train_seg_semisup_classthresh_mt against train_seg_semisup_mask_mt, each command as a process of
its own, synthetic data, `--arch resnet101_deeplab_imagenet --freeze_bn`, the same crop and batch, the img/s line of the LAST epoch of
each log, the two commands alternating twice. Prints one JSON line at the end. There is no threshold on any figure.
    python tools/cthresh_bench.py [--rounds 5] [--calls 50] [--end_to_end] [--e2e_iters 40]
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

# (N, C, (h, w), (H, W), align_corners): Pascal VOC on DeepLab v2, Cityscapes
SHAPES = [(10, 21, (41, 41), (321, 321), True), (4, 19, (65, 129), (512, 1024), True)]


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_stats(l0, l1, size, align, mask, um0, um1, thr):
    """teacher logits f32 (N,C,h,w) x 2, mask bool (N,1,H,W), um0 / um1 f32 (N,1,H,W), thr f32 (C,) -> (pass bits (N,H,W),
    n_valid, sum conf, sum_c q_c (C,), N_pred (C,), N_pass (C,)) over the valid pixels"""
    C = l0.shape[1]
    u = torch.where(mask, F.interpolate(l1, size=size, mode='bilinear', align_corners=align),
                    F.interpolate(l0, size=size, mode='bilinear', align_corners=align))
    q = torch.softmax(u, dim=1)
    conf, k = q.max(dim=1)
    valid = torch.where(mask, um1 >= 0.5, um0 >= 0.5)[:, 0]
    passed = conf >= thr[k]
    vf = valid.to(q.dtype)
    return (passed, valid.sum(), (conf * vf).sum(), (q * vf[:, None]).sum(dim=(0, 2, 3)),
            torch.bincount(k[valid], minlength=C), torch.bincount(k[valid & passed], minlength=C))


def launch_times(a, dev):
    results = []
    gen = mask_gen.BoxMaskGenerator(0.5, invert=True)
    for n, c, lo, size, align in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + c)
        ls, l0, l1 = [torch.randn((n, c) + lo, generator=g, device=dev) * 3 for _ in range(3)]
        ranges = ops.ranges_to_device(gen.generate_ranges(n, size, rng=np.random.RandomState(n + c)), dev)
        mask = ops.boxmask_rasterize(ranges, size, True) >= 0.5
        um0 = (torch.rand((n, 1) + size, generator=g, device=dev) > 0.1).float()
        um1 = (torch.rand((n, 1) + size, generator=g, device=dev) > 0.1).float()
        grad = torch.zeros_like(ls)
        ct = ops.ClassThresholds(c, dev, ema=0.999, floor=0.0, ceil=0.97)
        thr = torch.linspace(0.2, 0.6, c, device=dev)
        ct.thr.copy_(thr)
        fixed = ops.ConsistencyConfig(mode='mix', loss_fn='var', conf_thresh=0.4, align_corners=align)
        per_class = ops.ConsistencyConfig(mode='mix', loss_fn='var', conf_thresh=0.97, align_corners=align, class_thresh=ct)
        kw = dict(ranges=ranges, um0=um0, um1=um1)

        def run_fixed():
            grad.zero_()
            return ops.consistency_fused(fixed, ls, l0, l1, size, grad, **kw)

        def run_cthresh():
            grad.zero_()
            ct.update()
            ct.thr.copy_(thr)                     # (the same thresholds every call: the update above moved them)
            return ops.consistency_fused(per_class, ls, l0, l1, size, grad, **kw)

        def run_cthresh_timed():
            grad.zero_()
            ct.update()
            return ops.consistency_fused(per_class, ls, l0, l1, size, grad, **kw)

        routes = {'fixed': run_fixed, 'cthresh': run_cthresh_timed, 'torch': lambda: torch_stats(l0, l1, size, align, mask, um0, um1, thr)}
        run_cthresh()
        torch.cuda.synchronize()
        tab = ct.iteration_table().cpu().numpy().astype(np.uint64)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ref = routes['torch']()
        torch.cuda.synchronize()
        res = {'shape': [n, c, list(lo), list(size)], 'torch_peak_bytes': int(torch.cuda.max_memory_allocated(dev) - base),
               'n_valid': [int(tab[0]), int(ref[1])],
               'pass_count_difference_from_torch': int(np.abs(tab[2 + 2 * c:].astype(np.int64) - ref[5].cpu().numpy()).sum()),
               'pred_count_difference_from_torch': int(np.abs(tab[2 + c:2 + 2 * c].astype(np.int64) - ref[4].cpu().numpy()).sum()),
               'mean_conf': [float(tab[1]) / 2.0 ** 24 / float(tab[0]), float(ref[2]) / float(ref[1])]}
        del ref
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, f in routes.items():                                        # alternating: all see the same machine
                f()
                times[k].append(timed_ms(f, a.calls if k != 'torch' else max(1, a.calls // 5)))
            print('{} round {}: {}'.format(res['shape'], r, {k: round(v[-1], 4) for k, v in times.items()}), flush=True)
        for k in routes:
            res[k + '_ms_median'] = float(np.median(times[k]))
            res[k + '_ms_min'], res[k + '_ms_max'] = min(times[k]), max(times[k])
        res['cthresh_minus_fixed_ms'] = res['cthresh_ms_median'] - res['fixed_ms_median']
        res['fixed_spread_ms'] = res['fixed_ms_max'] - res['fixed_ms_min']
        print(res, flush=True)
        results.append(res)
    return results


def end_to_end(a):
    """img/s of the last epoch of each command, each in a process of its own"""
    out = {}
    common = ['--job_desc', 'bench', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', str(a.e2e_batch),
              '--crop_size', a.e2e_crop, '--learning_rate', '3e-5', '--lr_sched', 'poly', '--num_epochs', '3', '--iters_per_epoch',
              str(a.e2e_iters), '--synthetic_val_batches', '1']
    names = ('train_seg_semisup_mask_mt', 'train_seg_semisup_classthresh_mt')
    for name in names + names:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.join(REPO, name + '.py')] + common
            proc = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.e2e_timeout)
            if proc.returncode != 0:
                raise SystemExit('{} ended with {}:\n{}'.format(name, proc.returncode, proc.stdout.decode()[-2000:]))
            log = open(os.path.join(tmp, 'results', name, 'log_bench.txt')).read()
        rates = [float(v) for v in re.findall(r'-- ([\d.]+) img/s', log)]
        print(name, 'img/s per epoch', rates, re.findall(r'-- class thresholds tau=[\d.]+', log), flush=True)
        out.setdefault(name, []).append(rates[-1])
    return {'crop': a.e2e_crop, 'batch': a.e2e_batch, 'iters_per_epoch': a.e2e_iters, 'img_per_s_last_epoch': out,
            'classthresh_over_cutmix': float(np.mean(out[names[1]]) / np.mean(out[names[0]]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--end_to_end', action='store_true')
    ap.add_argument('--e2e_crop', default='321,321')
    ap.add_argument('--e2e_batch', type=int, default=10)
    ap.add_argument('--e2e_iters', type=int, default=40)
    ap.add_argument('--e2e_timeout', type=int, default=280)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cthresh_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    result = {'rounds': a.rounds, 'calls_per_round': a.calls, 'launches': launch_times(a, dev)}
    if a.end_to_end:
        torch.cuda.synchronize()
        result['end_to_end'] = end_to_end(a)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
