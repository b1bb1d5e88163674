"""Cross-pseudo-supervision labels on the device: what one batch of label maps costs, and what the CPS command makes of it.

Per-batch time of the one-launch label kernel (ops.cps_labels, csrc/cps.hip) at 10 x 21 x 41x41 -> 321x321 and 4 x 19 x 65x129 ->
512x1024, with a box table, both validity maps and `--conf_thresh` 0 (the CPS default) and 0.6, against the same labels in torch
operations on the same device in the same run, alternating, by device events:
    torch  four F.interpolate to (N, C, H, W), two `where` by the mask, two softmax / max passes, the compares. It lives here, not in
           the package: it is the yardstick. Its peak memory (torch.cuda.max_memory_allocated over one call, above what was allocated
           before it) is recorded too.
Per route and shape: a warm-up call, then `--rounds` rounds of `--calls` calls; ms per batch as the median over the rounds with the
smallest and largest round. The labels of the two routes are compared first (labels that differ are counted: the torch route
interpolates in another order). The byte floor -- at most 12 bytes read (mask or nothing, two validity maps) and 2 written per output
pixel at 8 TB/s, the low-resolution logits counted once -- is printed beside the times.

End-to-end (`--end_to_end`): img/s of train_seg_semisup_cps against train_seg_semisup_mask_mt, each command as a process of its own,
synthetic data, `--arch resnet101_deeplab_imagenet --freeze_bn`, the same crop and batch, the img/s line of the LAST epoch of each log
(the first epoch carries the warm-up), the two commands alternating twice. Prints one JSON line at the end. There is no threshold on
any figure.
    python tools/cps_bench.py [--rounds 5] [--calls 50] [--end_to_end] [--e2e_iters 40]
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
HBM_BYTES_PER_S = 8e12


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_cps_labels(logits, size, align, mask, um0, um1, tau):
    """four f32 (N,C,h,w) logit tensors, mask bool (N,1,H,W), um0 / um1 f32 (N,1,H,W) -> (label_a, label_b uint8 (N,H,W), int64[4])"""
    valid = torch.where(mask, um1 >= 0.5, um0 >= 0.5)[:, 0]
    labels, kept, preds = [], [], []
    for l0, l1 in ((logits[0], logits[1]), (logits[2], logits[3])):
        u = torch.where(mask, F.interpolate(l1, size=size, mode='bilinear', align_corners=align),
                        F.interpolate(l0, size=size, mode='bilinear', align_corners=align))
        pred = u.argmax(dim=1)
        keep = valid & (torch.softmax(u, dim=1).max(dim=1)[0] >= tau) if tau > 0 else valid
        labels.append(torch.where(keep, pred, torch.full_like(pred, 255)).to(torch.uint8))
        kept.append(keep.sum())
        preds.append(pred)
    stats = torch.stack([valid.sum(), kept[0], kept[1], (valid & (preds[0] == preds[1])).sum()])
    return labels[0], labels[1], stats


def label_times(a, dev):
    results = []
    gen = mask_gen.BoxMaskGenerator(0.5, invert=True)
    for n, c, lo, size, align in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + c)
        logits = [torch.randn((n, c) + lo, generator=g, device=dev) * 3 for _ in range(4)]
        ranges = ops.ranges_to_device(gen.generate_ranges(n, size, rng=np.random.RandomState(n + c)), dev)
        mask = ops.boxmask_rasterize(ranges, size, True) >= 0.5
        um0 = (torch.rand((n, 1) + size, generator=g, device=dev) > 0.1).float()
        um1 = (torch.rand((n, 1) + size, generator=g, device=dev) > 0.1).float()
        out = (torch.empty((n,) + size, dtype=torch.uint8, device=dev), torch.empty((n,) + size, dtype=torch.uint8, device=dev))
        stats = torch.empty(4, dtype=torch.int64, device=dev)
        pixels = n * size[0] * size[1]
        floor_bytes = pixels * (8 + 2) + 4 * logits[0].numel() * 4 + ranges.numel() * 4           # two validity maps, two label maps
        res = {'shape': [n, c, list(lo), list(size)], 'byte_floor_us': floor_bytes / HBM_BYTES_PER_S * 1e6,
               'byte_floor_with_a_float_mask_us': (floor_bytes + 4 * pixels) / HBM_BYTES_PER_S * 1e6}
        for tau in (0.0, 0.6):
            tag = 'tau{}'.format(tau)
            routes = {'hip': lambda: ops.cps_labels(*logits, size, ranges=ranges, um0=um0, um1=um1, conf_thresh=tau,
                                                    align_corners=align, labels_out=out, stats_out=stats),
                      'torch': lambda: torch_cps_labels(logits, size, align, mask, um0, um1, tau)}
            got = [t.clone() for t in routes['hip']()]
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            ref = routes['torch']()
            torch.cuda.synchronize()
            res[tag] = {'torch_peak_bytes': int(torch.cuda.max_memory_allocated(dev) - base),
                        'labels_differing_from_torch': int((ref[0] != got[0]).sum() + (ref[1] != got[1]).sum()),
                        'stats': got[2].cpu().tolist(), 'torch_stats': ref[2].cpu().tolist()}
            del ref
            times = {k: [] for k in routes}
            for r in range(a.rounds):
                for k, f in routes.items():                                        # alternating: both see the same machine
                    times[k].append(timed_ms(f, a.calls if k != 'torch' else max(1, a.calls // 5)))
                print('{} {} round {}: {}'.format(res['shape'], tag, r, {k: round(v[-1], 4) for k, v in times.items()}), flush=True)
            for k in routes:
                res[tag][k + '_ms_median'] = float(np.median(times[k]))
                res[tag][k + '_ms_min'], res[tag][k + '_ms_max'] = min(times[k]), max(times[k])
            res[tag]['share_of_byte_floor'] = res['byte_floor_us'] / (res[tag]['hip_ms_median'] * 1e3)
        print(res, flush=True)
        results.append(res)
    return results


def end_to_end(a):
    """img/s of the last epoch of each command, each in a process of its own"""
    out = {}
    common = ['--job_desc', 'bench', '--synthetic', '--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', str(a.e2e_batch),
              '--crop_size', a.e2e_crop, '--learning_rate', '3e-5', '--lr_sched', 'poly', '--num_epochs', '3', '--iters_per_epoch',
              str(a.e2e_iters), '--synthetic_val_batches', '1']
    names = ('train_seg_semisup_mask_mt', 'train_seg_semisup_cps')
    for name in names + names:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.join(REPO, name + '.py')] + common
            proc = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.e2e_timeout)
            if proc.returncode != 0:
                raise SystemExit('{} ended with {}:\n{}'.format(name, proc.returncode, proc.stdout.decode()[-2000:]))
            log = open(os.path.join(tmp, 'results', name, 'log_bench.txt')).read()
        rates = [float(v) for v in re.findall(r'-- ([\d.]+) img/s', log)]
        print(name, 'img/s per epoch', rates, re.findall(r'-- pseudo-label agreement=[\d.]+%', log), flush=True)
        out.setdefault(name, []).append(rates[-1])
    return {'crop': a.e2e_crop, 'batch': a.e2e_batch, 'iters_per_epoch': a.e2e_iters, 'img_per_s_last_epoch': out,
            'cps_over_cutmix': float(np.mean(out[names[1]]) / np.mean(out[names[0]]))}


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
        raise SystemExit('cps_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    result = {'rounds': a.rounds, 'calls_per_round': a.calls, 'labels': label_times(a, dev)}
    if a.end_to_end:
        torch.cuda.synchronize()
        result['end_to_end'] = end_to_end(a)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
