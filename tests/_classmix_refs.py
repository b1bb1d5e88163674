"""Test helper: the fp64 restatement, in plain numpy, of the ClassMix mask (csrc/classmix.hip) -- bilinear upsample in fp64 (the
restatement tests/_tta_refs.py holds against torch), argmax, the classes present, the chosen half by sorting (key, class), the mask --
and the cases the CPU and GPU tests share. Nothing here imports the product."""
import functools

import numpy as np

import _tta_refs as T

# the fp32 interpolation of N(0,1) logits stays within 1e-6 of its fp64 restatement (csrc/tta_math.hpp); ten times that
MARGIN = 1e-5


def bits(classes):
    out = 0
    for c in classes:
        out |= 1 << int(c)
    return out


def classmix(logits, keys, size, align_corners, valid=None):
    """logits (n,c,h,w), keys (n,c) float64, valid optional (n,H,W) -> dict(pred uint8 (n,H,W), present / chosen: python ints per
    sample (64-bit sets), mask float32 (n,1,H,W), gap: the smallest top-two gap of the upsampled logits over all pixels (inf for one
    class))"""
    up = T.upsample(logits, size, align_corners)
    n, c = up.shape[:2]
    pred = up.argmax(axis=1).astype(np.uint8)
    if c > 1:
        top = np.partition(up, c - 2, axis=1)
        gap = float((top[:, c - 1] - top[:, c - 2]).min())
    else:
        gap = float('inf')
    present, chosen = [], []
    mask = np.zeros((n, 1) + tuple(size), dtype=np.float32)
    for i in range(n):
        ok = np.ones(pred[i].shape, dtype=bool) if valid is None else (np.asarray(valid[i]) != 0)
        classes = sorted(set(pred[i][ok].tolist()))
        k = (len(classes) + 1) // 2
        first = sorted(classes, key=lambda cls: (keys[i, cls], cls))[:k]
        present.append(bits(classes))
        chosen.append(bits(first))
        mask[i, 0] = (ok & np.isin(pred[i], first)).astype(np.float32)
    return dict(pred=pred, present=present, chosen=chosen, mask=mask, gap=gap)


def as_int64(sets):
    """64-bit sets as the int64 words ops.classmix_mask's sets_out holds (bit 63 is the sign bit)"""
    return np.array(sets, dtype=np.uint64).astype(np.int64)


# name -> (n, c, (h, w), (H, W), align_corners, seed). N(0,1) logits; the seeds were searched on the CPU (tests/test_classmix_cpu.py
# re-checks them) so that the fp64 top-two gap is at least MARGIN at EVERY pixel.
#   main_*  1353 pixels per sample: not a multiple of 64, wave and workgroup tails; both corner conventions
#   c64     +4 on class 63 of sample 1 and the smallest key there: bit 63 present and chosen
#   ident   the low-resolution size is the output size: no interpolation
#   slots   131841 pixels per sample: 129 slot words per sample, more than one per lane of the wave that ORs them
CASES = {
    'main_ac': (3, 21, (5, 7), (33, 41), True, 0),
    'main_nac': (3, 21, (5, 7), (33, 41), False, 0),
    'c1': (3, 1, (5, 7), (33, 41), True, 0),
    'c2': (3, 2, (5, 7), (33, 41), True, 0),
    'c64': (3, 64, (5, 7), (33, 41), True, 0),
    'ident': (2, 7, (17, 19), (17, 19), True, 0),
    'slots': (2, 19, (33, 65), (257, 513), True, 1306),
}


def case_inputs(name, seed=None):
    n, c, lo, size, align, case_seed = CASES[name]
    rng = np.random.RandomState(case_seed if seed is None else seed)
    logits = rng.standard_normal((n, c) + lo).astype(np.float32)
    keys = rng.random_sample((n, c))
    if name == 'c64':
        logits[1, 63] += 4.0
        keys[1, 63] = -1.0
    return dict(logits=logits, keys=keys, size=size, align=align)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, reference), computed once and left unchanged"""
    inp = case_inputs(name)
    return inp, classmix(inp['logits'], inp['keys'], inp['size'], inp['align'])
