#!/usr/bin/env python
"""
Generate tests/golden/draw_params_single_size.json: parameter tables of `DeviceAugmenter.draw_params` for ONE source size per
batch, as drawn by the implementation BEFORE it accepted a per-sample list of sizes. tests/test_datapipe_cpu.py compares the
current implementation with them (a batch with one size must draw exactly what it always drew).

Run it on a checkout of the commit before the ragged staging path (the parent of the commit that added this file; the
committed tables were recorded from 8d27581, "Add the augmentation mean-teacher trainer with a fused affine-warp loss"):

    git worktree add /tmp/before <that commit>
    python tests/golden/make_draw_params_golden.py /tmp/before

The argument is the root of that checkout; its `cutmix_semisup_seg_amd.device_pipeline` is imported (no GPU, no built library
needed beyond what importing the package needs), this repository's is kept off the path. Run against the current tree it
reproduces the committed file as long as the property holds.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SEED, COLOUR_SEED, N = 11, 12, 5
CASES = [
    dict(crop=[48, 64], src=[60, 70], with_labels=False, cfg=dict(scale_hung=True, hflip=True, vflip=True, strong_colour=True)),
    dict(crop=[48, 48], src=[37, 53], with_labels=True, cfg=dict(hflip=True, vflip=True, hvflip=True)),
    dict(crop=[48, 64], src=[90, 20], with_labels=False,
         cfg=dict(rot_mag=30.0, max_scale=1.5, scale_non_uniform=True, strong_colour=True)),
    dict(crop=[48, 64], src=[20, 90], with_labels=False, cfg=dict(scale_hung=True, scale_non_uniform=True)),
]


def main(checkout):
    checkout = os.path.abspath(checkout)
    sys.path = [p for p in sys.path if os.path.abspath(p or '.') not in (REPO, HERE)]
    sys.path.insert(0, checkout)
    from cutmix_semisup_seg_amd import device_pipeline
    assert os.path.abspath(device_pipeline.__file__).startswith(checkout), device_pipeline.__file__
    out = []
    for c in CASES:
        aug = device_pipeline.DeviceAugmenter(c['crop'], MEAN, STD, rng=np.random.RandomState(SEED),
                                              colour_rng=np.random.RandomState(COLOUR_SEED), **c['cfg'])
        table = aug.draw_params(N, c['src'], with_labels=c['with_labels'])
        out.append(dict(c, seed=SEED, colour_seed=COLOUR_SEED, n=N, table=[[float(v) for v in r] for r in table]))
    with open(os.path.join(HERE, 'draw_params_single_size.json'), 'w') as f:
        json.dump(out, f, indent=0)
    print('wrote draw_params_single_size.json ({} cases) from {}'.format(len(out), checkout))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
