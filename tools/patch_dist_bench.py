"""Patch-distance analysis at the reference's Cityscapes geometry (intra_inter_class_patch_dist.py:188-189 quotes 0.25 s per
distance map and 0.03 s per argsort there, on the CPU): a synthetic pool of 512 x 1024 images, patch 225, 64 patches in chunks of
32, 1000 neighbours. Times, by device events, per (image, patch):
    map       the image side (load, 3 forward FFTs 1024 x 2048, box sums) plus per chunk spectrum product, inverse FFT and finish
    select    the two class selections (radix select of the intra and the inter keys, sort of the survivors)
and once per chunk and FFT size the patch spectra (load and 3 forward FFTs per pair), which every image of that size reuses.
Every round visits every image once after one warm-up visit; prints per-round times, then one JSON line with medians, spread
(max - min over the rounds) and the largest rounding residual seen. There is no threshold: nothing exists to regress against.
    python tools/patch_dist_bench.py [--images 4] [--patches 64] [--rounds 5] [--k 1000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cutmix_semisup_seg_amd import ops, patch_dist as pd  # noqa: E402
from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource  # noqa: E402

H, W, P, CHUNK = 512, 1024, 225, 32


def synthetic(n_images, rng):
    """smooth images and blocky label maps with void specks: what a street scene looks like to these kernels"""
    images, labels = [], []
    for _ in range(n_images):
        lo = rng.randint(0, 256, size=(H // 16 + 1, W // 16 + 1, 3))
        img = lo.repeat(16, 0).repeat(16, 1)[:H, :W] + rng.randint(-8, 9, size=(H, W, 3))
        images.append(np.clip(img, 0, 255).astype(np.uint8))
        lab = rng.randint(0, 19, size=(H // 32 + 1, W // 32 + 1)).repeat(32, 0).repeat(32, 1)[:H, :W].astype(np.uint8)
        lab[rng.uniform(size=(H, W)) < 0.02] = 255
        labels.append(lab)
    return images, labels


def elapsed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4)
    ap.add_argument('--patches', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--k', type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('patch_dist_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(0)
    images, labels = synthetic(a.images, rng)
    pool = ResidentPool(ArraySource(images, labels), range(a.images), dev, with_labels=True)
    rows = np.stack([rng.randint(0, a.images, a.patches), np.ones(a.patches, dtype=np.int64), rng.randint(0, H, a.patches),
                     rng.randint(0, W - 1, a.patches), np.zeros(a.patches, dtype=np.int64)], axis=1)
    rows[:, 4] = [labels[r[0]][r[2], r[3]] for r in rows]
    patches = pd.PatchSet(pool, rows, (P, P))
    chunks = pd.chunks_of(patches, CHUNK)
    residual_bits = torch.zeros((1,), dtype=torch.int64, device=dev)
    keys = [torch.empty((c.last - c.first, H * W), dtype=torch.int64, device=dev) for c in chunks]

    def maps(sample_i):
        img = pd._ImageSide(pool, sample_i, patches.patch_shape)
        for c, kbuf in zip(chunks, keys):
            pd._finish_chunk(img, c, residual_bits, keys=kbuf)
        return img

    def selections(img):
        for c, kbuf in zip(chunks, keys):
            cls = patches.cls[c.first:c.last]
            ops.select_k_smallest(kbuf, a.k, labels=img.labels, cls=cls)
            ops.select_k_smallest(kbuf, a.k, labels=img.labels, cls=cls, inter=True)

    # warm-up: the first visit loads every code object and grows the allocator's pools. Then the patch spectra alone (once per
    # chunk and FFT size): a visit with fresh caches against a visit with warm ones
    img = maps(0)
    selections(img)
    chunks[:] = pd.chunks_of(patches, CHUNK)
    spectra_ms, _ = elapsed_ms(lambda: maps(0))
    warm_ms, _ = elapsed_ms(lambda: maps(0))
    spectra_per_patch = (spectra_ms - warm_ms) / a.patches
    print('geometry: {} images {} x {}, patch {}, FFT {} x {}, {} patches in chunks of {}, k {}'.format(
        a.images, H, W, P, img.fft_shape[0], img.fft_shape[1], a.patches, CHUNK, a.k))
    print('visit with fresh patch spectra {:.1f} ms, with cached ones {:.1f} ms: spectra {:.3f} ms per patch, once per FFT size'.format(
        spectra_ms, warm_ms, spectra_per_patch))

    t_map, t_sel = [], []
    for r in range(a.rounds):
        m = s = 0.0
        for i in range(a.images):
            dm, img = elapsed_ms(lambda: maps(i))
            ds, _ = elapsed_ms(lambda: selections(img))
            m, s = m + dm, s + ds
        t_map.append(m / (a.images * a.patches))
        t_sel.append(s / (a.images * a.patches))
        print('round {}: map {:.4f} ms   two selections {:.4f} ms   per (image, patch)'.format(r, t_map[-1], t_sel[-1]), flush=True)
    residual = float(residual_bits.view(torch.float64).item())
    print(json.dumps({'geometry': [a.images, H, W, P], 'fft': list(img.fft_shape), 'patches': a.patches, 'chunk': CHUNK, 'k': a.k,
                      'rounds': a.rounds, 'map_ms_median': float(np.median(t_map)), 'map_ms_spread': max(t_map) - min(t_map),
                      'select_ms_median': float(np.median(t_sel)), 'select_ms_spread': max(t_sel) - min(t_sel),
                      'patch_spectra_ms_per_patch_once': spectra_per_patch, 'rounding_residual_max': residual,
                      'reference_cpu_ms': {'map': 250.0, 'argsort': 30.0}}))


if __name__ == '__main__':
    main()
