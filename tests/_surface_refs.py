"""Test helper: the cases tests/test_gpu_surface.py and tests/test_surface_cpu.py share, and the reference of the surface distances.

The reference is scipy only, MedPy's construction per class and image: the surface of a mask is
M & ~binary_erosion(M, generate_binary_structure(2, 1), border_value=0), the nearest surface pixel comes from
distance_transform_edt(~border, return_distances=False, return_indices=True), and the squared distance is recomputed from those indices
in int64, so it is exact. It uses none of the separable row / column form of csrc/surface_math.hpp. The integers (`stats`, the d2 maps)
have no tolerance; HD, HD95 and ASSD are numpy.percentile / max / mean over numpy.sqrt of them."""
import functools

import numpy as np
from scipy import ndimage

from _boundary_refs import IGNORE, blank_void, blobs, checkerboard, with_void

_CROSS = ndimage.generate_binary_structure(2, 1)


def surface(mask):
    """the pixels of a 2-D bool mask with a 4-neighbour outside it (the array's outside is outside)"""
    if not mask.any():
        return mask.copy()
    return mask & ~ndimage.binary_erosion(mask, _CROSS, border_value=0)


def directed_d2(src, dst):
    """int64 squared distance from every pixel of the bool map `src` to the nearest pixel of the non-empty bool map `dst`"""
    iy, ix = ndimage.distance_transform_edt(~dst, return_distances=False, return_indices=True)
    yy, xx = np.nonzero(src)
    return (yy.astype(np.int64) - iy[yy, xx]) ** 2 + (xx.astype(np.int64) - ix[yy, xx]) ** 2


def reference(truth, pred, c, ignore=IGNORE):
    """truth, pred (N,H,W) uint8 -> dict: stats (N,c,6) int64, sums (N,c,2) float64, d2_pred / d2_truth (N,H,W) int32, and the
    scores per pair hd / hd95 / assd (N,c) float64, NaN where the pair is not scored"""
    n, h, w = truth.shape
    stats = np.full((n, c, 6), -1, dtype=np.int64)
    sums = np.zeros((n, c, 2), dtype=np.float64)
    d2p = np.full((n, h, w), -1, dtype=np.int32)
    d2t = np.full((n, h, w), -1, dtype=np.int32)
    hd, hd95, assd = (np.full((n, c), np.nan) for _ in range(3))
    for i in range(n):
        t = truth[i]
        p = blank_void(t, pred[i], ignore) if ignore is not None else pred[i]
        void = (t == ignore) if ignore is not None else np.zeros(t.shape, dtype=bool)
        for cl in range(c):
            bs, bg = surface((p == cl) & ~void), surface((t == cl) & ~void)
            stats[i, cl, 0], stats[i, cl, 1] = bs.sum(), bg.sum()
            if not bs.any() or not bg.any():
                continue
            a, b = directed_d2(bs, bg), directed_d2(bg, bs)
            d2p[i][bs], d2t[i][bg] = a, b
            pooled = np.sort(np.concatenate([a, b]))
            m = len(pooled)
            lo = (19 * (m - 1)) // 20
            stats[i, cl, 2:] = a.max(), b.max(), pooled[lo], pooled[min(lo + 1, m - 1)]
            sums[i, cl] = np.sqrt(a).sum(), np.sqrt(b).sum()
            root = np.sqrt(pooled)
            hd[i, cl], hd95[i, cl] = root.max(), np.percentile(root, 95)
            assd[i, cl] = 0.5 * (np.sqrt(a).mean() + np.sqrt(b).mean())
    return dict(stats=stats, sums=sums, d2_pred=d2p, d2_truth=d2t, hd=hd, hd95=hd95, assd=assd)


def scored(stats):
    return (stats[..., 0] > 0) & (stats[..., 1] > 0)


def one_sided(stats):
    return (stats[..., 0] > 0) != (stats[..., 1] > 0)


def dataset(refs):
    """references of the batches of a data set -> dict of (c,) arrays: the mean of hd / hd95 / assd over the scored images of every
    class (NaN without one) and the pair counts"""
    out = {}
    for key in ('hd', 'hd95', 'assd'):
        v = np.concatenate([r[key] for r in refs], axis=0)
        cnt = (~np.isnan(v)).sum(axis=0)
        out[key] = np.where(cnt > 0, np.nansum(v, axis=0) / np.maximum(cnt, 1), np.nan)
    st = np.concatenate([r['stats'] for r in refs], axis=0)
    out['scored'], out['one_sided'] = scored(st).sum(axis=0).astype(np.int64), one_sided(st).sum(axis=0).astype(np.int64)
    return out


def lines(prefix, ds):
    """the seven lines eval_seg --surface_dist prints, from dataset()'s result"""
    out = []
    for name, key in (('HD95', 'hd95'), ('ASSD', 'assd'), ('HD', 'hd')):
        v = ds[key]
        head = v[~np.isnan(v)].mean() if (~np.isnan(v)).any() else float('nan')
        out.append('{} {}={:.3f}'.format(prefix, name, head))
        out.append('-- {} {}'.format(name, ', '.join('-' if np.isnan(x) else '{:.3f}'.format(x) for x in v)))
    out.append('-- surface pairs {} (one-sided {})'.format(', '.join(str(int(x)) for x in ds['scored']),
                                                           ', '.join(str(int(x)) for x in ds['one_sided'])))
    return out


# ------------------------------------------------------------------------------------------------------------------ maps
def _pair(shape, c, seed, void=False, sigma=3.0):
    truth = blobs(shape, c, seed, sigma=sigma)
    if void:
        truth = with_void(truth, seed + 1)
    return truth, blobs(shape, c, seed + 1000, sigma=min(sigma, 2.0))


def _one_pixel(hit):
    return np.zeros((1, 1, 1), dtype=np.uint8), np.full((1, 1, 1), 0 if hit else 1, dtype=np.uint8)


def _row_of_7():
    return np.array([[[0, 0, 1, 1, 1, 0, 0]]], dtype=np.uint8), np.array([[[0, 1, 1, 0, 0, 0, 1]]], dtype=np.uint8)


def _same():
    truth, _ = _pair((2, 33, 41), 5, 5, void=True)
    pred = truth.copy()
    pred[truth == IGNORE] = 0                       # what a network says under void pixels is anything
    return truth, pred


def _checker():
    truth = checkerboard((2, 33, 41))
    return truth, (1 - truth).astype(np.uint8)


def _tall():
    """blobs of the classes 0..3, and class 4 in the truth's first row and the prediction's last row only: d2 = 299^2 > 65535"""
    truth, pred = blobs((1, 300, 5), 4, 7), blobs((1, 300, 5), 4, 1007, sigma=2.0)
    truth[0, 0, 1:4] = 4
    pred[0, -1, 2] = 4
    return truth, pred


def _ends(shape, axis):
    """class 1 in the truth's first row (column) and the prediction's last one only, class 0 elsewhere"""
    truth, pred = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    if axis == 0:
        truth[0, 0, :], pred[0, -1, :] = 1, 1
    else:
        truth[0, :, 0], pred[0, :, -1] = 1, 1
    return truth, pred


def _far_corner():
    """class 1: single pixels at opposite corners. Class 2: a prediction pixel whose nearest truth pixels are 5 away in its row and 5
    away in its column (a tie). Class 3: the same with the column's pixel one row further off, where the walk must have stopped."""
    truth, pred = np.zeros((1, 67, 130), dtype=np.uint8), np.zeros((1, 67, 130), dtype=np.uint8)
    truth[0, 0, 0], pred[0, 66, 129] = 1, 1
    pred[0, 20, 30] = 2
    truth[0, 20, 35], truth[0, 25, 30] = 2, 2
    pred[0, 40, 90] = 3
    truth[0, 40, 95], truth[0, 46, 90] = 3, 3
    return truth, pred


def _isolated(counts, shape=(1, 20, 30)):
    """class 1 as counts[0] isolated truth pixels and counts[1] isolated prediction pixels on a background of class 0"""
    truth, pred = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    spots = [(y, x) for y in range(1, shape[1], 3) for x in range(1, shape[2], 3)]
    rng = np.random.RandomState(9)
    for m, k in ((truth, counts[0]), (pred, counts[1])):
        for j in rng.permutation(len(spots))[:k]:
            m[0][spots[j]] = 1
    return truth, pred


def _one_sided():
    truth, pred = _pair((2, 33, 41), 5, 12)
    truth, pred = truth.copy(), pred.copy()
    pred[pred == 3] = 0                             # class 3 is never predicted
    truth[1][truth[1] == 4] = 1                     # image 1 has no class 4
    return truth, pred


CASES = {
    'one_pixel': lambda: _one_pixel(False) + (2,),
    'one_pixel_hit': lambda: _one_pixel(True) + (2,),
    'row_of_7': lambda: _row_of_7() + (2,),
    'c2': lambda: _pair((2, 33, 41), 2, 2) + (2,),
    'c5_void': lambda: _pair((2, 33, 41), 5, 3, void=True) + (5,),
    'c21_void': lambda: _pair((3, 67, 130), 21, 4, void=True) + (21,),       # crosses 64 and 128; the last image is all void
    'same': lambda: _same() + (5,),
    'checkerboard': lambda: _checker() + (2,),
    'wide': lambda: _pair((1, 5, 300), 2, 6) + (2,),
    'tall': lambda: _tall() + (5,),
    'very_tall': lambda: _ends((1, 4200, 3), 0) + (2,),
    'very_wide': lambda: _ends((1, 3, 4200), 1) + (2,),
    'far_corner': lambda: _far_corner() + (4,),
    'n21': lambda: _isolated((10, 11)) + (2,),
    'n2': lambda: _isolated((1, 1)) + (2,),
    'one_sided': lambda: _one_sided() + (5,),
    'c64': lambda: _pair((2, 40, 50), 64, 11, sigma=1.0) + (64,),
}
SMALL = ('one_pixel', 'one_pixel_hit', 'row_of_7', 'c5_void', 'c21_void', 'wide', 'tall', 'far_corner', 'n21', 'one_sided')


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, reference): computed once per process, shared; treat as read-only"""
    truth, pred, c = CASES[name]()
    inp = dict(truth=np.ascontiguousarray(truth, dtype=np.uint8), pred=np.ascontiguousarray(pred, dtype=np.uint8), c=c)
    ref = reference(inp['truth'], inp['pred'], c)
    for a in list(inp.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp, ref


def sums_close(got, ref_sums, stats):
    """relative (n + 2) 2^-52 of the reference's fp64 sum, n that direction's surface count: the worst case of adding n square roots
    that are each correctly rounded or one ulp off, in any order"""
    bound = (stats[..., :2].astype(np.float64) + 2.0) * 2.0 ** -52 * np.abs(ref_sums)
    return bool((np.abs(got - ref_sums) <= bound).all())
