"""ClassMix masks on the device: what one batch of masks costs, and what the ClassMix command makes of it.

Per-batch time of the two-launch mask (ops.classmix_mask, csrc/classmix.hip) at 10 x 21 x 41x41 -> 321x321 and 4 x 19 x 65x129 ->
512x1024, against two yardsticks on the same device in the same run, alternating, by device events:
    torch  the same mask in torch operations: F.interpolate to (N, C, H, W), argmax, per sample `unique` (a host synchronisation
           each), the half with the smallest keys, `isin`. It lives here, not in the package: it is the yardstick. Its peak memory
           (torch.cuda.max_memory_allocated over one call, above what was allocated before it) is recorded too.
    vote   ops.tta_vote with one view and `pred`: the kernel with the same gather pattern that only writes the uint8 prediction. The
           mask pair additionally writes 4 and re-reads 1 byte per pixel and reduces the sets.
Per route and shape: a warm-up call, then `--rounds` rounds of `--calls` calls; ms per batch as the median over the rounds with the
smallest and largest round. The masks of the first two routes are compared first (pixels that differ are counted: the torch route
interpolates in another order).

End-to-end (`--end_to_end`): img/s of train_seg_semisup_classmix_mt against train_seg_semisup_mask_mt, each command as a process of its
own, synthetic data, `--arch resnet101_deeplab_imagenet --freeze_bn`, the same crop and batch, the img/s line of the LAST epoch of each
log (the first epoch carries the warm-up), the two commands alternating twice. Prints one JSON line at the end. There is no threshold
on any figure.
    python tools/classmix_bench.py [--rounds 5] [--calls 50] [--end_to_end] [--e2e_iters 40]
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


def torch_classmix(logits, keys, size, align):
    """logits f32 (N,C,h,w), keys f64 (N,C) on the device -> f32 (N,1,H,W)"""
    pred = F.interpolate(logits, size=size, mode='bilinear', align_corners=align).argmax(dim=1)
    masks = []
    for i in range(pred.shape[0]):
        classes = torch.unique(pred[i])                                        # the host waits here: the shape depends on the data
        k = (int(classes.numel()) + 1) // 2
        first = classes[torch.argsort(keys[i][classes], stable=True)[:k]]
        masks.append(torch.isin(pred[i], first))
    return torch.stack(masks)[:, None].float()


def mask_times(a, dev):
    results = []
    gen = mask_gen.ClassMixGenerator()
    for n, c, lo, size, align in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + c)
        logits = torch.randn((n, c) + lo, generator=g, device=dev)
        keys = torch.from_numpy(gen.generate_params(n, c, rng=np.random.RandomState(n + c))).to(dev)
        out = torch.empty((n, 1) + size, dtype=torch.float32, device=dev)
        pred = torch.empty((n,) + size, dtype=torch.uint8, device=dev)
        routes = {'hip': lambda: ops.classmix_mask(logits, keys, size, align_corners=align, out=out),
                  'torch': lambda: torch_classmix(logits, keys, size, align),
                  'vote': lambda: ops.tta_vote([logits], [False], c, size, align_corners=align, pred=pred)}
        got = routes['hip']().clone()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ref = routes['torch']()
        torch.cuda.synchronize()
        res = {'shape': [n, c, list(lo), list(size)], 'torch_peak_bytes': int(torch.cuda.max_memory_allocated(dev) - base),
               'pixels_differing_from_torch': int((ref != got).sum()),
               'share_of_ones': [round(float(v), 4) for v in got.mean(dim=(1, 2, 3)).cpu()],
               'bytes_hip_writes_per_pixel': 5}
        del ref
        routes['vote']()
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, f in routes.items():                                        # alternating: all see the same machine
                times[k].append(timed_ms(f, a.calls if k != 'torch' else max(1, a.calls // 5)))
            print('{} round {}: {}'.format(res['shape'], r, {k: round(v[-1], 4) for k, v in times.items()}), flush=True)
        for k in routes:
            res[k + '_ms_median'] = float(np.median(times[k]))
            res[k + '_ms_min'], res[k + '_ms_max'] = min(times[k]), max(times[k])
        print(res, flush=True)
        results.append(res)
    return results


def end_to_end(a):
    """img/s of the last epoch of each command, each in a process of its own"""
    out = {}
    common = ['--job_desc', 'bench', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', str(a.e2e_batch),
              '--crop_size', a.e2e_crop, '--learning_rate', '3e-5', '--lr_sched', 'poly', '--num_epochs', '3', '--iters_per_epoch',
              str(a.e2e_iters), '--synthetic_val_batches', '1']
    names = ('train_seg_semisup_mask_mt', 'train_seg_semisup_classmix_mt')
    for name in names + names:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.join(REPO, name + '.py')] + common
            proc = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.e2e_timeout)
            if proc.returncode != 0:
                raise SystemExit('{} ended with {}:\n{}'.format(name, proc.returncode, proc.stdout.decode()[-2000:]))
            log = open(os.path.join(tmp, 'results', name, 'log_bench.txt')).read()
        rates = [float(v) for v in re.findall(r'-- ([\d.]+) img/s', log)]
        print(name, 'img/s per epoch', rates, flush=True)
        out.setdefault(name, []).append(rates[-1])
    return {'crop': a.e2e_crop, 'batch': a.e2e_batch, 'iters_per_epoch': a.e2e_iters, 'img_per_s_last_epoch': out,
            'classmix_over_cutmix': float(np.mean(out[names[1]]) / np.mean(out[names[0]]))}


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
        raise SystemExit('classmix_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    result = {'rounds': a.rounds, 'calls_per_round': a.calls, 'masks': mask_times(a, dev)}
    if a.end_to_end:
        torch.cuda.synchronize()
        result['end_to_end'] = end_to_end(a)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
