#!/usr/bin/env python
"""
Generate the data-only fixtures of the augmentation mean-teacher trainer's tests:

    tests/golden/aug_cli.json     the command-line surface of the reference's trainer (train_seg_semisup_aug_mt.py:515-567), read
                                  off the click command of the reference's own module
    tests/golden/aug_pairs.json   pair matrices computed by the reference's datapipe/affine.py functions (cat_nx2x3, inv_nx2x3,
                                  translation / scale / rotation / flip_xyd matrices, cv_to_torch) from recorded draw parameters

    python tests/golden/make_aug_golden.py <path of a checkout of the reference>

Needs the reference's sources; its outputs (small JSON files holding only settings and recorded numbers) are committed and are
all the tests read.
"""
import importlib.util
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

# recorded draw parameters: crop (H, W); positions (y, x) of both views; the resize factors (x, y) of view 1; flip flags [x, y, d]
# per view; for the rotate / scale crop the scales (y, x) and angles of both views, the common centre (y, x), view 1's offset
CROP_CASES = [
    dict(crop=[33, 41], pos0=[5, 9], pos1=[12, 3], size1=[33, 41], flips=[[0, 0, 0], [0, 0, 0]]),
    dict(crop=[33, 41], pos0=[0, 7], pos1=[3, 0], size1=[33, 41], flips=[[1, 0, 0], [0, 1, 0]]),
    dict(crop=[40, 40], pos0=[11, 2], pos1=[4, 9], size1=[40, 40], flips=[[1, 1, 1], [0, 0, 1]]),
    dict(crop=[33, 41], pos0=[20, 30], pos1=[8, 13], size1=[47, 59], flips=[[0, 0, 0], [1, 0, 0]]),
    dict(crop=[40, 40], pos0=[6, 6], pos1=[17, 1], size1=[27, 27], flips=[[0, 1, 0], [1, 1, 1]]),
]
WARP_CASES = [
    dict(crop=[33, 41], scales=[[1.2, 1.2], [1.2, 1.2]], thetas=[0.3, 0.3], centre=[60.5, 71.25], offset1=[4.0, -7.0],
         flips=[[0, 0, 0], [0, 0, 0]]),
    dict(crop=[40, 40], scales=[[0.8, 1.1], [1.3, 0.7]], thetas=[-0.5, 0.2], centre=[55.0, 48.5], offset1=[-16.0, 9.0],
         flips=[[1, 0, 1], [0, 1, 0]]),
]


def load_affine(ref):
    spec = importlib.util.spec_from_file_location('ref_affine', os.path.join(ref, 'datapipe', 'affine.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pair_matrices(affine):
    out = []
    for c in CROP_CASES:
        crop = np.array(c['crop'])
        pos = np.array([c['pos0'][::-1], c['pos1'][::-1]])
        factors = np.append(np.array([[1, 1]]), crop[None, ::-1].astype(float) / np.array(c['size1'])[None, ::-1], axis=0)
        xf = affine.cat_nx2x3(affine.translation_matrices((factors - 1.0) * 0.5), affine.scale_matrices(factors),
                              affine.translation_matrices(-pos), affine.identity_xf(2))
        out.append((c, crop, xf))
    for c in WARP_CASES:
        crop = np.array(c['crop'])
        centre = np.array([c['centre'], c['centre']])
        off = np.stack([np.zeros((2,)), np.array(c['offset1'])])
        xf = affine.cat_nx2x3(affine.translation_matrices(crop[None, ::-1] * 0.5), affine.translation_matrices(off[:, ::-1]),
                              affine.rotation_matrices(np.array(c['thetas'])), affine.scale_matrices(np.array(c['scales'])[:, ::-1]),
                              affine.translation_matrices(-centre[:, ::-1]))
        out.append((c, crop, xf))
    res = []
    for c, crop, xf in out:
        f = np.array(c['flips']) != 0
        xf = affine.cat_nx2x3(affine.flip_xyd_matrices(f, tuple(crop)), xf)
        cv01 = affine.cat_nx2x3(xf[1:2], affine.inv_nx2x3(xf[0:1]))
        t01 = affine.cv_to_torch(cv01, tuple(crop))[0].astype(np.float32)
        res.append(dict(params=c, xf_cv=[[[float(v) for v in r] for r in m] for m in xf],
                        xf0_to_1=[[float(v) for v in r] for r in t01]))
    return res


def main(ref):
    ref = os.path.abspath(ref)
    # keep the repository root (which holds a same-named drop-in script) OFF the path; the reference goes first
    sys.path = [p for p in sys.path if os.path.abspath(p or '.') not in (REPO, HERE)]
    sys.path.insert(0, ref)
    import click
    import train_seg_semisup_aug_mt as ref_trainer   # reference (the module body only defines the job and the click command)
    assert os.path.abspath(ref_trainer.__file__).startswith(ref)
    opts = []
    for prm in ref_trainer.experiment.params:
        kind = type(prm.type).__name__
        choices = list(prm.type.choices) if isinstance(prm.type, click.Choice) else None
        opts.append(dict(name=prm.name, opts=list(prm.opts), is_flag=bool(getattr(prm, 'is_flag', False)),
                         default=prm.default if not callable(prm.default) else None, type=kind, choices=choices))
    with open(os.path.join(HERE, 'aug_cli.json'), 'w') as f:
        json.dump(opts, f, indent=0, default=str)
    print('wrote aug_cli.json ({} options)'.format(len(opts)))
    pairs = pair_matrices(load_affine(ref))
    with open(os.path.join(HERE, 'aug_pairs.json'), 'w') as f:
        json.dump(pairs, f, indent=0)
    print('wrote aug_pairs.json ({} pairs)'.format(len(pairs)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
