"""The ISIC 2017 converter's area resize on the device: what one launch costs, and where a conversion's time goes.

Per-launch time of the resize to 248 x 248 at (1, 767, 1022, 3) -- the smallest ISIC image --, (1, 4499, 6748, 3) -- the largest -- and
(8, 1504, 2016, 3) -- a same-size run of a chunk. Two routes on the same device in the same run, alternating, by device events:
    hip      ops.resize_area_u8: csrc/resize.hip, one launch, integers only
    library  the same definition through the library: the source as fp64, two matmuls with the dense weight matrices, then the
             division with ties to even in int64 and a cast, with its peak allocation. Every intermediate is a whole number below
             2^53, so the route is exact too. (Dividing in fp64 and calling torch.round is not: the device's fp64 quotient of an
             exact half came out one ulp high on 7 of 1 476 096 values at 8 x 1504 x 2016 and rounded up, where the integer rule --
             checked there in Python integers -- rounds to even.) It lives here, not in the package: it is the yardstick.
and against the HBM floor of a kernel that reads the source bytes once, at --hbm_tb_s. Per route and shape: a warm-up call, then
`--rounds` rounds of `--calls` calls; ms per launch as the median over the rounds with the spread (max - min). The two outputs are
compared first (pixels that differ are counted).

Phase split (`--converter_images N`): N full-size samples (4499 x 6748 JPEGs, one encoded image under N names, three quarters in the
training archive) are written to a temporary directory and converted by convert_isic.convert_archives in this process; the decode /
device / encode-and-write seconds it reports are recorded. Prints one JSON line at the end. There is no threshold on any figure.
    python tools/resize_bench.py [--rounds 5] [--calls 20] [--converter_images 64]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
import zipfile

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, REPO)
from cutmix_semisup_seg_amd import ops  # noqa: E402

SHAPES = [(1, 767, 1022, 3), (1, 4499, 6748, 3), (8, 1504, 2016, 3)]
TARGET = (248, 248)


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def weight_matrix(L, Lo, dev):
    o, i = torch.arange(Lo, dtype=torch.int64, device=dev)[:, None], torch.arange(L, dtype=torch.int64, device=dev)[None, :]
    return (torch.minimum((i + 1) * Lo, (o + 1) * L) - torch.maximum(i * Lo, o * L)).clamp_(min=0).double()


def library_resize(x, wy, wx):
    """x uint8 (N,H,W,C), wy f64 (ho,H), wx f64 (wo,W) -> uint8 (N,ho,wo,C)"""
    n, h, w, c = x.shape
    rows = torch.matmul(wy, x.double().reshape(n, h, w * c))                   # (N, ho, W C)
    num = torch.matmul(wx, rows.reshape(n * wy.shape[0], w, c))                # (N ho, wo, C)
    num, den = num.to(torch.int64), h * w
    q = torch.div(num, den, rounding_mode='floor')
    r = num - q * den
    q += (2 * r > den) | ((2 * r == den) & (q % 2 == 1))
    return q.to(torch.uint8).reshape(n, wy.shape[0], wx.shape[0], c)


def kernel_times(a, dev):
    results = []
    ho, wo = TARGET
    for shape in SHAPES:
        n, h, w, c = shape
        x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(h), device=dev)
        out = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=dev)
        wy, wx = weight_matrix(h, ho, dev), weight_matrix(w, wo, dev)
        routes = {'hip': lambda: ops.resize_area_u8(x, ho, wo, out=out)}
        src_bytes = n * h * w * c
        res = {'shape': list(shape), 'target': [ho, wo], 'source_mib': round(src_bytes / 2 ** 20, 1),
               'hbm_floor_ms': src_bytes / (a.hbm_tb_s * 1e12) * 1e3}
        got = routes['hip']().clone()
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            lib = library_resize(x, wy, wx)
            torch.cuda.synchronize()
            res['library_peak_mib'] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
            res['pixels_differing_from_library'] = int((lib != got).sum())
            routes['library'] = lambda: library_resize(x, wy, wx)
            del lib
        except Exception as e:                                                 # the yardstick is missing, the figure stands
            res['library_error'] = '{}: {}'.format(type(e).__name__, str(e).splitlines()[0] if str(e) else '')
            print('library route not taken:', res['library_error'], flush=True)
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, f in routes.items():                                        # alternating: both see the same machine
                times[k].append(timed_ms(f, a.calls if k == 'hip' else max(1, a.calls // 5)))
            print('{} round {}: {}'.format(shape, r, {k: round(v[-1], 4) for k, v in times.items()}), flush=True)
        for k in routes:
            res[k + '_ms_median'] = float(np.median(times[k]))
            res[k + '_ms_spread'] = max(times[k]) - min(times[k])
        res['hip_fraction_of_floor'] = res['hbm_floor_ms'] / res['hip_ms_median']
        res['hip_gb_s'] = src_bytes / res['hip_ms_median'] / 1e6
        print(res, flush=True)
        results.append(res)
        del x, out, wy, wx
        torch.cuda.empty_cache()
    return results


def converter_split(a):
    """one conversion of fabricated full-size archives -> the converter's own phase seconds"""
    from PIL import Image
    from cutmix_semisup_seg_amd import convert_isic
    h, w = 4499, 6748
    rng = np.random.RandomState(0)
    x = rng.randint(0, 256, size=(h // 16 + 1, w // 16 + 1, 3)).repeat(16, 0).repeat(16, 1)[:h, :w].astype(np.uint8)
    x += rng.randint(0, 8, size=x.shape).astype(np.uint8) * (x < 240)
    yy, xx = np.mgrid[:h, :w]
    y = (((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 3)) ** 2 < 1).astype(np.uint8) * 255
    t0 = time.time()
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', quality=90)
    x_jpg = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(y).save(buf, 'PNG')
    y_png = buf.getvalue()
    n_train = a.converter_images * 3 // 4
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        zips = os.path.join(tmp, 'zips')
        os.makedirs(zips)
        k = 0
        for (x_zip, y_zip, y_folder, _), count in zip(convert_isic.ARCHIVES, (n_train, a.converter_images - n_train)):
            with zipfile.ZipFile(os.path.join(zips, x_zip), 'w') as zx, zipfile.ZipFile(os.path.join(zips, y_zip), 'w') as zy:
                for _ in range(count):
                    zx.writestr('{}/ISIC_{:07d}.jpg'.format(x_zip[:-4], k), x_jpg)
                    zy.writestr('{}/ISIC_{:07d}_segmentation.png'.format(y_folder, k), y_png)
                    k += 1
        fabricate_s = time.time() - t0
        with open(os.path.join(tmp, 'semantic_segmentation.cfg'), 'w') as f:
            f.write('[paths]\nisic2017={}\n'.format(os.path.join(tmp, 'out', 'isic2017.zip')))
        os.chdir(tmp)
        try:
            t0 = time.time()
            res = convert_isic.convert_archives(zips, '248,248')
            wall = time.time() - t0
        finally:
            os.chdir(cwd)
    return {'images': a.converter_images, 'size': [h, w], 'jpeg_mib': round(len(x_jpg) / 2 ** 20, 2), 'mask_png_kib': round(len(y_png) / 1024, 1),
            'fabricate_s': fabricate_s, 'wall_s': wall, 'seconds': res['seconds']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--hbm_tb_s', type=float, default=8.0, help='peak HBM bandwidth the floor is taken against')
    ap.add_argument('--converter_images', type=int, default=0, help='also convert this many fabricated full-size samples')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resize_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    result = {'rounds': a.rounds, 'calls_per_round': a.calls, 'hbm_tb_s': a.hbm_tb_s, 'kernel': kernel_times(a, dev)}
    if a.converter_images > 0:
        torch.cuda.synchronize()
        result['converter'] = converter_split(a)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
