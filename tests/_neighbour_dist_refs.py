"""Test-side restatements of the neighbouring-patch distances (the reference's patch_dist.py:57-104), on exact integers and written
from the formula, not from the product's route (no neighbour-difference planes shared between directions, no running sums):

    D2[dir][i, j] = sum over the p_h x p_w window at (i, j) and the channels of (c - neighbour of c in direction dir)^2

with c the image symmetric-padded by (p - 1) // 2 + 1 per axis, its outermost ring left off. brute_neighbour_d2 is the p_h * p_w
loop in numpy that the device is held to; torch_neighbour_d2 states the same as a gather-pad and an int64 summed-area table from
torch.cumsum, runs on whatever device its input is on, and is the yardstick of tools/neighbour_dist_bench.py."""
import numpy as np

OFFSETS = ((0, -1), (0, 1), (-1, 0), (1, 0))            # left, right, up, down: (dy, dx) of the neighbour


def symmetric_indices(n, before, after):
    """source indices of an axis of length n under numpy's `symmetric` padding, any number of reflections"""
    m = np.mod(np.arange(-before, n + after), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def brute_neighbour_d2(image, patch_shape):
    """uint8 (H, W, 3) -> int64 (4, H, W)"""
    image = np.asarray(image)
    h, w = image.shape[:2]
    ph, pw = int(patch_shape[0]), int(patch_shape[1])
    a, b = (ph - 1) // 2, (pw - 1) // 2
    rows, cols = symmetric_indices(h, a + 1, a + 1), symmetric_indices(w, b + 1, b + 1)
    padded = image.astype(np.int64)[rows][:, cols]                           # (H + 2a + 2, W + 2b + 2, 3)
    hp, wp = h + ph - 1, w + pw - 1
    centre = padded[1:1 + hp, 1:1 + wp]
    out = np.zeros((4, h, w), dtype=np.int64)
    for k, (dy, dx) in enumerate(OFFSETS):
        neighbour = padded[1 + dy:1 + dy + hp, 1 + dx:1 + dx + wp]
        sq = ((centre - neighbour) ** 2).sum(axis=2)
        for u in range(ph):
            for v in range(pw):
                out[k] += sq[u:u + h, v:v + w]
    return out


def brute_box_sum(plane, box):
    """int64 (H - b_h + 1, W - b_w + 1): the b_h * b_w loop"""
    plane = np.asarray(plane).astype(np.int64)
    bh, bw = box
    ho, wo = plane.shape[0] - bh + 1, plane.shape[1] - bw + 1
    out = np.zeros((ho, wo), dtype=np.int64)
    for u in range(bh):
        for v in range(bw):
            out += plane[u:u + ho, v:v + wo]
    return out


def torch_neighbour_d2(image, patch_shape):
    """uint8 torch (H, W, 3), on any device -> int64 (4, H, W): gather-pad, four squared difference planes, one cumsum SAT each"""
    import torch
    h, w = int(image.shape[0]), int(image.shape[1])
    ph, pw = int(patch_shape[0]), int(patch_shape[1])
    a, b = (ph - 1) // 2, (pw - 1) // 2
    rows = torch.from_numpy(symmetric_indices(h, a + 1, a + 1)).to(image.device)
    cols = torch.from_numpy(symmetric_indices(w, b + 1, b + 1)).to(image.device)
    padded = image.to(torch.int64)[rows][:, cols]
    hp, wp = h + ph - 1, w + pw - 1
    centre = padded[1:1 + hp, 1:1 + wp]
    maps = []
    for dy, dx in OFFSETS:
        sq = ((centre - padded[1 + dy:1 + dy + hp, 1 + dx:1 + dx + wp]) ** 2).sum(dim=2)
        c = torch.nn.functional.pad(sq.cumsum(0).cumsum(1), (1, 0, 1, 0))
        maps.append(c[ph:, pw:] - c[:-ph, pw:] - c[ph:, :-pw] + c[:-ph, :-pw])
    return torch.stack(maps)


def golden_agrees(golden_map, d2):
    """the criterion that ties a float64 map of the reference to the exact integers: where the reference is finite its square, in
    grey levels, rounds to D2 (a margin of 1/2 against a reference error of at most a few 1e-7 at the golden sizes); where it is
    NaN (a summed-area table that cancelled to just below zero) D2 is 0. -> (ok, worst |g^2 * 65025 - D2| over the finite part)"""
    g, d2 = np.asarray(golden_map, dtype=np.float64), np.asarray(d2)
    finite = np.isfinite(g)
    if np.isinf(g).any():
        return False, float('inf')
    sq = g[finite] ** 2 * 65025.0
    ok = np.array_equal(np.rint(sq), d2[finite].astype(np.float64)) and bool((d2[~finite] == 0).all())
    return ok, float(np.abs(sq - d2[finite]).max()) if finite.any() else 0.0
