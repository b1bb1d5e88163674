"""Test-side numpy restatements for the patch-distance analysis: the int64 brute force of the squared distance maps, the stable
class selection, the anchor choice and the whole class_distances loop on exact integers. Written from the formulae, independent
of the product's code path (no FFT, no keys): what the device computes is held to these."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

OFFSETS = np.array([[0, -1], [0, 1], [-1, 0], [1, 0]])


def pads(patch_shape):
    return (patch_shape[0] - 1) // 2, (patch_shape[1] - 1) // 2


def padded(image, patch_shape):
    ph, pw = pads(patch_shape)
    return np.pad(image.astype(np.int64), [[ph, ph], [pw, pw], [0, 0]], mode='symmetric')


def cut_patch(image, patch_shape, yx):
    """the patch centred on yx of the symmetric-padded image, int64 (p_h, p_w, 3)"""
    ip = padded(image, patch_shape)
    return ip[yx[0]:yx[0] + patch_shape[0], yx[1]:yx[1] + patch_shape[1]]


def brute_d2(image, patches, positions=None):
    """int64 (N, H, W): sum over the window of (Ipad - Q)^2, every position; or (N, len(positions)) at the given (y, x) only"""
    patches = np.asarray(patches).astype(np.int64)
    shape = patches.shape[1:3]
    ip = padded(image, shape)
    if positions is not None:
        out = np.zeros((len(patches), len(positions)), dtype=np.int64)
        for k, (y, x) in enumerate(positions):
            win = ip[y:y + shape[0], x:x + shape[1]]
            out[:, k] = ((win[None] - patches) ** 2).sum(axis=(1, 2, 3))
        return out
    win = sliding_window_view(ip, (shape[0], shape[1], 3))[:, :, 0]          # (H, W, p_h, p_w, 3)
    out = np.zeros((len(patches),) + win.shape[:2], dtype=np.int64)
    for n, q in enumerate(patches):
        for y in range(win.shape[0]):                                       # row by row: bounded memory
            out[n, y] = ((win[y] - q[None]) ** 2).sum(axis=(1, 2, 3))
    return out


def select_stable(values, mask, k):
    """indices of the k smallest `values` among `mask`, ties by ascending index (a stable argsort)"""
    order = np.argsort(values, kind='stable')
    return order[mask[order]][:k]


def class_selection(d2_map, labels, cls, k):
    """-> (intra, inter): int64 (m, [D2, y, x]) ascending, ties by flat index"""
    flat, lab = d2_map.reshape(-1), labels.reshape(-1)
    out = []
    for mask in (lab == cls, (lab != cls) & (lab != 255)):
        idx = select_stable(flat, mask, k)
        out.append(np.stack([flat[idx], idx // d2_map.shape[1], idx % d2_map.shape[1]], axis=1).astype(np.int64))
    return out


def choose_anchors(labels_of, sample_indices, n_patches, patch_shape, rng):
    """rows [img_i, dir, y, x, cls]: boundary pixels per image and direction, border filter pad + 1 < i < H - (pad + 1), one draw"""
    ph, pw = pads(patch_shape)
    rows = []
    for img_i in sample_indices:
        y = np.asarray(labels_of(int(img_i))).astype(np.int64)
        H, W = y.shape
        for d, (dy, dx) in enumerate(OFFSETS):
            for i in range(1, H - 1):
                for j in range(1, W - 1):
                    c, nb = y[i, j], y[i + dy, j + dx]
                    if c == 255 or nb == 255 or nb == c:
                        continue
                    if ph + 1 < i < H - (ph + 1) and pw + 1 < j < W - (pw + 1):
                        rows.append([int(img_i), d, i, j, c])
    rows = np.array(rows, dtype=np.int64).reshape(-1, 5)
    return rows[rng.permutation(len(rows))[:n_patches]]


def class_distances(images, labels, sample_indices, rows, patch_shape, k):
    """the reference's class_distances loop on exact integers. images / labels: dicts by sample index. Ties: (D2, visit order,
    flat index). -> dict of the eight lists plus boundary_dists; dists are sqrt(D2) / 255."""
    n = len(rows)
    anchors = np.stack([cut_patch(images[int(r[0])], patch_shape, r[2:4]) for r in rows])
    negatives = np.stack([cut_patch(images[int(r[0])], patch_shape, r[2:4] + OFFSETS[r[1]]) for r in rows])
    same = {s: [None] * n for s in ('intra', 'inter')}
    other = {s: [np.zeros((0, 4), dtype=np.int64) for _ in range(n)] for s in ('intra', 'inter')}     # [D2, img, y, x]
    for img_i in sample_indices:
        img_i = int(img_i)
        d2 = brute_d2(images[img_i], anchors)
        for p in range(n):
            intra, inter = class_selection(d2[p], labels[img_i], rows[p][4], k)
            for side, sel in (('intra', intra), ('inter', inter)):
                sel = np.concatenate([sel[:, :1], np.full((len(sel), 1), img_i, dtype=np.int64), sel[:, 1:]], axis=1)
                if img_i == rows[p][0]:
                    same[side][p] = sel
                else:
                    both = np.concatenate([other[side][p], sel], axis=0)
                    other[side][p] = both[np.argsort(both[:, 0], kind='stable')[:k]]
    res = {}
    for where, lists in (('same_image', same), ('other_image', other)):
        for side in ('intra', 'inter'):
            name = '{}_{}_class'.format(where, side)
            res[name + '_dists'] = [None if a is None else np.sqrt(a[:, 0].astype(np.float64)) / 255.0 for a in lists[side]]
            res[name + '_coords'] = [None if a is None else a[:, 1:] for a in lists[side]]
    res['boundary_dists'] = np.sqrt(((anchors - negatives) ** 2).sum(axis=(1, 2, 3)).astype(np.float64)) / 255.0
    return res
