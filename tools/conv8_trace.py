#!/usr/bin/env python
"""Cycle trace of the eight-phase convolution (csrc/conv8.hip, variant 92 = variant 90 with stamps): where the cycles of a
workgroup go -- tables, first loads, K loop (per K tile), epilogue.
    python tools/conv8_trace.py [shape-name substrings ...]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cutmix_semisup_seg_amd import ops
from cutmix_semisup_seg_amd._lib import lib
from conv8_check import PERF, make, run, timeit

names = [a for a in sys.argv[1:]]
cases = [c for c in PERF if not names or any(s in c[0] for s in names)]
for case in cases:
    t = make(case)
    epi = 'relu' if case[5] < 1024 else 'res_relu'
    out = run(t, epi, 99)
    nwg = 2048
    buf = torch.zeros(nwg * 64, dtype=torch.int32, device='cuda:0')
    for _ in range(2):
        run(t, epi, 90, out=out)
    torch.cuda.synchronize()
    t_plain = timeit(lambda: run(t, epi, 90, out=out), 10)
    lib.cms_conv_set_trace(buf.data_ptr(), nwg)
    run(t, epi, 92, out=out)
    torch.cuda.synchronize()
    lib.cms_conv_set_trace(None, 0)
    tr = buf.cpu().numpy().view(np.uint32).reshape(nwg, 64)[:, :16].astype(np.int64)
    tiles = tr[tr[:, 12] > 0]                        # (workgroups traced, 16)
    if len(tiles) == 0:
        print(case[0], 'no workgroups traced')
        continue
    d = lambda a, b: ((tiles[:, a] - tiles[:, b]) & 0xffffffff)
    kt = tiles[:, 12]
    print('== {}: {:.1f} us; {} tiles, {:.1f} K tiles each'.format(case[0], t_plain, len(tiles), kt.mean()))
    print('   tables {:.0f} | first loads {:.0f} | K loop {:.0f} = {:.0f} per K tile'.format(
        d(1, 0).mean(), d(2, 1).mean(), d(3, 2).mean(), (d(3, 2) / kt).mean()))
    print('   stage operands {:.0f} | build tile {:.0f} | stores {:.0f}   (total {:.0f})'.format(
        d(6, 3).mean(), d(7, 6).mean(), d(8, 7).mean(), d(8, 0).mean()))
