"""Evaluation with hole filling at the ISIC 2017 configuration's geometry (BASELINE config 5: logits 10 x 2 x 248 x 248, identity
size, uint8 truth): EvaluatorIoU(2, True).sample_logits on the device (csrc/fillholes.hip) against the host path it replaced,
restated here: argmax map, then per image device-to-host copy, scipy.ndimage.binary_fill_holes, host-to-device copy and
ops.confusion. Both legs run in one process, alternated round by round after warm-up; a leg's time is the host clock around
`calls` evaluator calls that end in a device synchronise. Prints per-round times, then one JSON line with the medians and the
spread (max - min over the rounds of each leg).
    python tools/fill_holes_bench.py [--rounds 7] [--calls 200] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cutmix_semisup_seg_amd import ops  # noqa: E402
from cutmix_semisup_seg_amd.evaluation import EvaluatorIoU  # noqa: E402

N, C, H, W = 10, 2, 248, 248


def blobs(gen):
    """smooth random logits: predictions made of blobs with holes, as a segmentation network's are (white noise would be all seams)"""
    lo = torch.randn(N, C, 16, 16, generator=gen)
    up = torch.nn.functional.interpolate(lo, size=(H, W), mode='bicubic', align_corners=False)
    return (up + 0.15 * torch.randn(N, C, H, W, generator=gen)).contiguous()


class HostPath(object):
    """what EvaluatorIoU(2, True).sample_logits did before the device kernel: one host round trip per image"""

    def __init__(self, dev):
        self.cm = torch.zeros((2, 2), dtype=torch.int64, device=dev)

    def sample_logits(self, logits, truth, ignore_value=255):
        from scipy.ndimage import binary_fill_holes
        _, pred = ops.argmax_confusion(logits, None, 2, truth.shape[-2:], align_corners=True, want_pred=True)
        for i in range(pred.shape[0]):
            p = pred[i].cpu().numpy()
            filled = torch.from_numpy(binary_fill_holes(p != 0).astype(np.uint8)).to(pred.device, non_blocking=True)
            ops.confusion(truth[i, 0].contiguous(), filled, 2, ignore_index=ignore_value, cm=self.cm)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3        # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fill_holes_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    logits = blobs(gen).to(dev)
    truth = (torch.rand(N, 1, H, W, generator=gen) < 0.3).to(torch.uint8)
    truth[:, :, :4, :] = 255
    truth = truth.to(dev)

    device_ev, host_ev = EvaluatorIoU(2, True), HostPath(dev)
    dev_call = lambda: device_ev.sample_logits(logits, truth, ignore_value=255)       # noqa: E731
    host_call = lambda: host_ev.sample_logits(logits, truth, ignore_value=255)        # noqa: E731
    for _ in range(a.warmup):
        dev_call()
        host_call()
    torch.cuda.synchronize()
    # same inputs, same number of calls: the two legs must have counted the same pixels
    same = torch.equal(device_ev._cm(), host_ev.cm)
    _, pred = ops.argmax_confusion(logits, None, 2, (H, W), want_pred=True)
    filled, _ = ops.fill_holes(pred)
    n_filled = int((filled != pred).sum())
    print('inputs: {} x {} x {} x {}; pixels filled per call: {}; confusion matrices equal: {}'.format(N, C, H, W, n_filled, same))
    if not same:
        raise SystemExit('fill_holes_bench: device and host legs disagree; timings withheld')

    td, th = [], []
    for r in range(a.rounds):
        td.append(timed(dev_call, a.calls))
        th.append(timed(host_call, a.calls))
        print('round {}: device {:.3f} ms   host {:.3f} ms   (per call of {} images)'.format(r, td[-1], th[-1], N), flush=True)
    res = {'geometry': [N, C, H, W], 'rounds': a.rounds, 'calls_per_round': a.calls, 'pixels_filled_per_call': n_filled,
           'device_ms_median': float(np.median(td)), 'device_ms_min': min(td), 'device_ms_max': max(td),
           'host_ms_median': float(np.median(th)), 'host_ms_min': min(th), 'host_ms_max': max(th)}
    res['spread_ms'] = max(max(td) - min(td), max(th) - min(th))
    res['device_faster_by_more_than_spread'] = bool(res['host_ms_median'] - res['device_ms_median'] > res['spread_ms']
                                                    and max(td) < min(th))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
