"""The ragged staging kernel (cms_stage_batch, csrc/stage.hip: every batch sample gathered from its own entry of an HBM-resident
pool) against the dense staging kernel cms_augment_batch AS BUILT FROM AN EARLIER COMMIT -- never against this tree's own build:

    git worktree add /tmp/before <commit before the ragged path>  &&  python /tmp/before/cutmix-semisup-seg_amd/build.py
    python tools/stage_bench.py --dense_lib /tmp/before/cutmix-semisup-seg_amd/csrc/libcutmixseg_hip.so

That library is loaded with ctypes beside the current one. Input for both legs: 10 uint8 sources of 375 x 500 (a pool whose entries
all have that size, index = 0..9) -> 10 x 3 x 321 x 321 bf16 with labels and validity mask, Hung scale crop + horizontal flip, the
SAME seeded parameter table; `colour` adds the student view. Before anything is timed, the outputs of the earlier commit's dense
kernel, this tree's dense kernel and the ragged kernel (images, mask, labels, and the three luminance pre-passes) are compared with
torch.equal; a difference stops the tool.

Timing: device events around `launches` back-to-back launches of one leg (a round), legs alternated, `rounds` rounds each after
a warm-up round; microseconds per launch. A round of 25 000 launches of ~10 us is a quarter of a second. At this size a launch
moves bytes_per_launch() (printed) -- microseconds of HBM time -- so the figure is launch + per-wave latency, the same for both
legs. Then one whole iteration's staging through DeviceAugmenter.stage (one supervised + two unsupervised batches with the colour
view: host draws, uploads, luminance pre-pass, gather), host clock around iterations that end in a device synchronise; with
--step_ms (bench.py's `ms_per_step` of the same session) its share of the step is printed.
Prints per-round times, then one JSON line (also written to --out).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cutmix_semisup_seg_amd import _lib                                          # noqa: E402
from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter             # noqa: E402
from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource     # noqa: E402

N, HS, WS, H, W = 10, 375, 500, 321, 321
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def bytes_per_launch(colour):
    """what one launch has to move: every source pixel a crop touches at most once from HBM (<= the whole pool entry), the bf16
    image planes (x 2 with the colour view), the fp32 mask, the uint8 labels"""
    px = N * H * W
    return dict(read_at_most=N * HS * WS * 4, written=px * (3 * 2 * (2 if colour else 1) + 4 + 1))


def load_dense(path):
    lib = C.CDLL(os.path.abspath(path))
    if os.path.samefile(path, _lib.LIB_PATH) or hasattr(lib, 'cms_stage_batch'):
        sys.exit('--dense_lib must be a build of a commit BEFORE the ragged path (it exports cms_stage_batch, or is this tree\'s)')
    lib.cms_augment_batch.restype = lib.cms_augment_luma.restype = C.c_int
    lib.cms_augment_batch.argtypes = [C.POINTER(_lib.AugmentDesc), C.c_void_p]
    lib.cms_augment_luma.argtypes = [C.POINTER(_lib.AugmentDesc), C.c_void_p, C.c_void_p]
    return lib


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3          # microseconds per launch


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), spread=float(max(v) - min(v)), rounds=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dense_lib', required=True, help='libcutmixseg_hip.so built from a commit before the ragged path')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--launches', type=int, default=25000)
    ap.add_argument('--luma_launches', type=int, default=1000)
    ap.add_argument('--iterations', type=int, default=150)
    ap.add_argument('--step_ms', type=float, default=0.0, help="bench.py's ms_per_step of the same session")
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('stage_bench needs a GPU: a time taken anywhere else says nothing')
    dense = load_dense(args.dense_lib)
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (N, HS, WS, 3), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 21, (N, HS, WS), generator=g).to(torch.uint8)
    src_d, lab_d = src.to(dev), lab.to(dev)
    pool = ResidentPool(ArraySource(list(src.numpy()), list(lab.numpy())), range(N), dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = dict(shape='{} x {} x {} uint8 -> {} x 3 x {} x {} bf16'.format(N, HS, WS, N, H, W), launches_per_round=args.launches)

    for colour in (False, True):
        key = 'colour' if colour else 'plain'
        aug = DeviceAugmenter((H, W), MEAN, STD, scale_hung=True, hflip=True, strong_colour=colour, out_dtype=torch.bfloat16,
                              rng=np.random.RandomState(1), colour_rng=np.random.RandomState(2))
        params = aug.draw_params(N, (HS, WS), with_labels=True)
        params[:, 14] = 0.45                                  # a fixed contrast pivot: the image kernel alone is timed
        p_dev = torch.from_numpy(params).to(dev)
        out0 = torch.empty((N, 3, H, W), dtype=torch.bfloat16, device=dev)
        out1 = torch.empty_like(out0) if colour else None
        mask = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
        labs = torch.empty((N, 1, H, W), dtype=torch.uint8, device=dev)
        idx = torch.arange(N, dtype=torch.int32, device=dev)
        a, s = _lib.AugmentDesc(), _lib.StageDesc()
        a.src, a.src_labels, a.hs, a.ws = src_d.data_ptr(), lab_d.data_ptr(), HS, WS
        s.pool_img, s.pool_labels = pool.image_buffer.data_ptr(), pool.label_buffer.data_ptr()
        s.entries, s.index, s.n_entries = pool.table_dev.data_ptr(), idx.data_ptr(), len(pool)
        for d in (a, s):
            d.out0, d.out1 = out0.data_ptr(), (out1.data_ptr() if colour else None)
            d.out_labels, d.out_mask, d.params = labs.data_ptr(), mask.data_ptr(), p_dev.data_ptr()
            for i in range(3):
                d.mean[i], d.std_[i] = MEAN[i], STD[i]
            d.n, d.h, d.w, d.out_dtype = N, H, W, _lib.BF16
        outs = [t for t in (out0, out1, mask, labs) if t is not None]
        legs = dict(dense_before=lambda: dense.cms_augment_batch(C.byref(a), stream),
                    dense_now=lambda: _lib.fn['cms_augment_batch'](C.byref(a), stream),
                    ragged=lambda: _lib.fn['cms_stage_batch'](C.byref(s), stream))
        got = {}
        for name, call in legs.items():
            for t in outs:
                t.zero_()
            assert call() == 0, name
            torch.cuda.synchronize()
            got[name] = [t.clone() for t in outs]
        lum = torch.zeros(N, device=dev)
        lumas = dict(dense_before=lambda: dense.cms_augment_luma(C.byref(a), C.c_void_p(lum.data_ptr()), stream),
                     dense_now=lambda: _lib.fn['cms_augment_luma'](C.byref(a), C.c_void_p(lum.data_ptr()), stream),
                     ragged=lambda: _lib.fn['cms_stage_luma'](C.byref(s), C.c_void_p(lum.data_ptr()), stream))
        for name, call in lumas.items():
            lum.zero_()
            assert call() == 0, name
            torch.cuda.synchronize()
            got[name].append(lum.clone())
        for name in ('dense_now', 'ragged'):
            if not all(torch.equal(x, y) for x, y in zip(got['dense_before'], got[name])):
                sys.exit('{}: the outputs of `{}` differ from the earlier commit\'s dense kernel; nothing timed'.format(key, name))
        for name in ('dense_before', 'ragged'):
            timed(legs[name], args.launches // 5)
        t = dict(dense_before=[], ragged=[])
        for r in range(args.rounds):
            for name in ('dense_before', 'ragged'):
                t[name].append(timed(legs[name], args.launches))
            print('{} round {}: dense (earlier commit) {:.3f} us, ragged {:.3f} us'.format(key, r, t['dense_before'][-1],
                                                                                         t['ragged'][-1]), flush=True)
        tl = dict(dense_before=[], ragged=[])
        for name in tl:
            timed(lumas[name], args.luma_launches // 5)
        for r in range(3):
            for name in tl:
                tl[name].append(timed(lumas[name], args.luma_launches))
        result[key] = dict(outputs_bit_identical=True, bytes=bytes_per_launch(colour), dense_before_us=stats(t['dense_before']),
                           ragged_us=stats(t['ragged']), luma_dense_before_us=stats(tl['dense_before']),
                           luma_ragged_us=stats(tl['ragged']))

    aug = DeviceAugmenter((H, W), MEAN, STD, scale_hung=True, hflip=True, strong_colour=True, out_dtype=torch.bfloat16,
                          rng=np.random.RandomState(1), colour_rng=np.random.RandomState(2))
    ids = list(range(N))

    def iteration():
        aug.stage(pool, ids, True)
        aug.stage(pool, ids, False)
        aug.stage(pool, ids, False)
    for _ in range(20):
        iteration()
    torch.cuda.synchronize()
    its = []
    for r in range(5):
        t0 = time.perf_counter()
        for _ in range(args.iterations):
            iteration()
        torch.cuda.synchronize()
        its.append((time.perf_counter() - t0) / args.iterations * 1e3)
    result['iteration_staging_ms'] = stats(its)
    if args.step_ms > 0:
        result['step_ms'] = args.step_ms
        result['staging_share_of_step'] = float(np.median(its)) / args.step_ms
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
