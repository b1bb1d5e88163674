"""Test helper: the cases tests/test_gpu_boundary.py and tests/test_boundary_cpu.py share, and the reference of the boundary scores.

The reference is the construction of the Boundary IoU authors' code, per class: the band of width d of a class mask G is
G & ~binary_erosion(G, ones((3, 3)), iterations=d, border_value=0) (scipy). It does not use the separable row / column form of
csrc/boundary_math.hpp. The distance map is the same operator one iteration at a time: D(p) = 1 + the number of erosions p survives.
All of it is integer; nothing here has a tolerance."""
import functools

import numpy as np
from scipy import ndimage

IGNORE = 255
_S = np.ones((3, 3), dtype=bool)


def blank_void(truth, pred, ignore=IGNORE):
    """P: the prediction with every void pixel set to ignore"""
    return np.where(truth == ignore, ignore, pred).astype(np.uint8)


def band(mask, d):
    """the pixels of a class mask within Chebyshev distance d of its boundary (2-D bool)"""
    if not mask.any():
        return mask.copy()
    return mask & ~ndimage.binary_erosion(mask, _S, iterations=int(d), border_value=0)


def band_map(m, c, d):
    """(H,W) map -> bool: the union of the bands of the classes 0..c-1 (void pixels, value 255 >= c, belong to none)"""
    out = np.zeros(m.shape, dtype=bool)
    for cl in np.unique(m):
        if cl < c:
            out |= band(m == cl, d)
    return out


def dist_map(m, c):
    """(H,W) map -> uint8 min(D, 255), 0 where the value is no class"""
    out = np.zeros(m.shape, dtype=np.int64)
    for cl in np.unique(m):
        if cl >= c:
            continue
        e = m == cl
        while e.any():
            out += e
            e = ndimage.binary_erosion(e, _S, border_value=0)
    return np.minimum(out, 255).astype(np.uint8)


def confusion(truth, pred, c, widths, ignore=IGNORE):
    """truth, pred (N,H,W) uint8, widths (N,K) -> bcm (K,c+1,c+1), tcm (K,c,c) int64"""
    widths = np.asarray(widths)
    n, k = widths.shape
    bcm = np.zeros((k, c + 1, c + 1), dtype=np.int64)
    tcm = np.zeros((k, c, c), dtype=np.int64)
    for i in range(n):
        t, p = truth[i], blank_void(truth[i], pred[i], ignore)
        live = t != ignore
        for j in range(k):
            bt, bp = band_map(t, c, widths[i, j]), band_map(p, c, widths[i, j])
            tq = np.where(bt, t, c).astype(np.int64)[live]
            pq = np.where(bp, p, c).astype(np.int64)[live]
            bcm[j] += np.bincount(tq * (c + 1) + pq, minlength=(c + 1) ** 2).reshape(c + 1, c + 1)
            in_t = bt & live
            tcm[j] += np.bincount(t[in_t].astype(np.int64) * c + p[in_t], minlength=c * c).reshape(c, c)
    return bcm, tcm


def dist_maps(truth, pred, c, ignore=IGNORE):
    dt = np.stack([dist_map(t, c) for t in truth])
    dp = np.stack([dist_map(blank_void(t, p, ignore), c) for t, p in zip(truth, pred)])
    return dt, dp


def boundary_iou(bcm):
    c = bcm.shape[-1] - 1
    diag = np.diagonal(bcm, axis1=-2, axis2=-1)[..., :c]
    union = bcm.sum(axis=-1)[..., :c] + bcm.sum(axis=-2)[..., :c] - diag
    return diag.astype(float) / np.maximum(union.astype(float), 1.0)


def plain_iou(cm):
    diag = np.diagonal(cm, axis1=-2, axis2=-1)
    union = cm.sum(axis=-1) + cm.sum(axis=-2) - diag
    return diag.astype(float) / np.maximum(union.astype(float), 1.0)


def width_px(spec, size):
    """an integer is pixels; a ratio r of the image's own diagonal is max(1, int(round(r * sqrt(h*h + w*w))))"""
    if isinstance(spec, int):
        return spec
    h, w = size
    return max(1, int(round(spec * np.sqrt(h * h + w * w))))


# ------------------------------------------------------------------------------------------------------------------ maps
def blobs(shape, c, seed, sigma=3.0):
    """argmax of c smoothed noise planes: a map of blobs"""
    rng = np.random.RandomState(seed)
    n, h, w = shape
    z = rng.standard_normal((n, c, h, w))
    z = ndimage.gaussian_filter(z, sigma=(0, 0, sigma, sigma), mode='nearest')
    return z.argmax(axis=1).astype(np.uint8)


def checkerboard(shape):
    n, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to(((yy + xx) & 1).astype(np.uint8), shape).copy()


def with_void(truth, seed):
    """void blocks in every sample, a void ring round an object in the first, and the last sample fully void (when there are three)"""
    rng = np.random.RandomState(seed)
    t = truth.copy()
    n, h, w = t.shape
    for i in range(n):
        for _ in range(3):
            y, x = rng.randint(0, h), rng.randint(0, w)
            t[i, y:y + rng.randint(1, 9), x:x + rng.randint(1, 9)] = IGNORE
    if h >= 20 and w >= 20:
        t[0, 5:16, 6:19] = IGNORE
        t[0, 7:14, 8:17] = 1
    if n >= 3:
        t[n - 1] = IGNORE
    return t


def _case(shape, c, widths, kind='blobs', void=False, pred='independent', seed=0):
    n = shape[0]
    if kind == 'blobs':
        truth = blobs(shape, c, seed)
    elif kind == 'constant':
        truth = np.full(shape, c - 1, dtype=np.uint8)
    elif kind == 'checker':
        truth = checkerboard(shape)
    elif kind == 'long_row':
        truth = np.zeros(shape, dtype=np.uint8)
        truth[0, shape[1] // 2, 3] = 1
    if void:
        truth = with_void(truth, seed + 1)
    p = truth.copy() if pred == 'same' else blobs(shape, c, seed + 1000, sigma=2.0)
    if pred == 'same':
        p[truth == IGNORE] = 0                      # what a network says under void pixels is anything
    w = np.asarray(widths, dtype=np.int32)
    if w.ndim == 1:
        w = np.broadcast_to(w[None], (n, w.shape[0])).copy()
    return dict(truth=truth, pred=p, c=c, widths=w)


CASES = {
    'one_pixel': lambda: _case((1, 1, 1), 2, [1]),
    'row_of_7': lambda: _case((1, 1, 7), 2, [1, 2, 5, 254], seed=1),
    'c2_k1': lambda: _case((2, 33, 41), 2, [2], seed=2),
    'c5_void': lambda: _case((2, 33, 41), 5, [1, 2, 5, 254], void=True, seed=3),
    # crosses 64 and 128 in both axes (67 rows > 64, 130 columns > 128); widths differ per sample, one of them >= max(H, W)
    'c21_void': lambda: _case((3, 67, 130), 21, [[1, 2, 5, 254], [3, 130, 7, 2], [5, 5, 5, 5]], void=True, seed=4),
    'c21_same': lambda: _case((3, 67, 130), 21, [5], pred='same', void=True, seed=5),
    'wide': lambda: _case((1, 5, 300), 2, [1, 5, 254], seed=6),
    'tall': lambda: _case((1, 300, 5), 5, [1, 2, 300 - 46], seed=7),
    'constant': lambda: _case((2, 33, 41), 2, [2, 254], kind='constant', pred='same'),
    'checkerboard': lambda: _case((2, 33, 41), 2, [1, 2], kind='checker', pred='same'),
    # a run of more than 2 * 255 + 64 equal pixels: the row pass gives up looking for its ends and stores the cap
    'long_row': lambda: _case((1, 3, 700), 2, [1, 254], kind='long_row', pred='same'),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, reference): computed once per process, shared; treat as read-only"""
    inp = CASES[name]()
    bcm, tcm = confusion(inp['truth'], inp['pred'], inp['c'], inp['widths'])
    dt, dp = dist_maps(inp['truth'], inp['pred'], inp['c'])
    for a in list(inp.values()) + [bcm, tcm, dt, dp]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp, dict(bcm=bcm, tcm=tcm, dist_truth=dt, dist_pred=dp)
