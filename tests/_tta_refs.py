"""Test helper: the fp64 restatement, in plain numpy, of the test-time augmentation kernels (csrc/tta.hip) -- the resize that makes a
view's input and the vote over the views' logits -- and the cases the CPU and GPU tests share. Nothing here imports the product."""
import functools

import numpy as np


# ------------------------------------------------------------------------------------------------------------------ bilinear taps
def taps(out_size, in_size, align_corners):
    """-> (i0, i1, w1) per output index: F.interpolate(mode='bilinear')'s source positions, in fp64"""
    d = np.arange(out_size, dtype=np.float64)
    if align_corners:
        src = d * ((in_size - 1) / (out_size - 1) if out_size > 1 else 0.0)
    else:
        src = np.maximum((d + 0.5) * (in_size / out_size) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, np.clip(src - i0, 0.0, 1.0)


def upsample(x, size, align_corners, flip=False):
    """x (..., h, w) -> (..., H, W) fp64. `flip`: x was computed on the mirrored input and is un-mirrored: the x taps point at the
    mirrored columns and keep their weights."""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[-2:]
    y0, y1, wy = taps(size[0], h, align_corners)
    x0, x1, wx = taps(size[1], w, align_corners)
    if flip:
        x0, x1 = w - 1 - x0, w - 1 - x1
    r0, r1 = x[..., y0, :], x[..., y1, :]
    a = (1.0 - wx) * r0[..., x0] + wx * r0[..., x1]
    b = (1.0 - wx) * r1[..., x0] + wx * r1[..., x1]
    wy = wy[:, None]
    return (1.0 - wy) * a + wy * b


def resize(x, size, flip=False):
    """cms_tta_resize: the align_corners=False bilinear sample at every output pixel, position and interpolation in fp64, no
    antialiasing; the result mirrored with `flip`"""
    out = upsample(x, size, False)
    return out[..., ::-1].copy() if flip else out


def interp_matrix(out_size, in_size, align_corners):
    """(out, in) matrix of the same interpolation: a second, gather-free formulation (used to check `upsample` against)"""
    i0, i1, w1 = taps(out_size, in_size, align_corners)
    m = np.zeros((out_size, in_size))
    np.add.at(m, (np.arange(out_size), i0), 1.0 - w1)
    np.add.at(m, (np.arange(out_size), i1), w1)
    return m


# ------------------------------------------------------------------------------------------------------------------ the vote
def softmax(v, axis):
    e = np.exp(v - v.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def vote(logits_list, flips, size, align_corners):
    """-> (score (n,c,H,W) fp64, pred (n,H,W) uint8, gap (n,H,W): best score minus runner-up; inf for one class).
    One view: the scores are its upsampled logits. More: the sum over the views of softmax(upsampled logits)."""
    ups = [upsample(l, size, align_corners, f) for l, f in zip(logits_list, flips)]
    score = ups[0] if len(ups) == 1 else sum(softmax(u, 1) for u in ups)
    pred = score.argmax(axis=1)
    if score.shape[1] > 1:
        top = np.sort(score, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(pred.shape, np.inf)
    return score, pred.astype(np.uint8), gap


def gap_bound(k):
    """An fp32 sum of k probabilities, each a few ulp off through interpolation, expf and the reciprocal, stays well inside this"""
    return 64 * k * 2.0 ** -24


def confusion(truth, pred, c, ignore=255):
    keep = (truth != ignore) & (truth < c)
    return np.bincount(truth[keep].astype(np.int64) * c + pred[keep], minlength=c * c).reshape(c, c)


# ------------------------------------------------------------------------------------------------------------------ shared cases
OUT = (2, 37, 53)                                           # n, H, W of the GPU vote cases
VIEW_SIZES = [(5, 7), (9, 13), (37, 53), (60, 80)]          # low-res, low-res, identity, larger than the output

# (k, C) -> (seed, align_corners): seeds searched on the CPU (tests/test_tta_cpu.py::test_vote_case_margins re-checks them) so that the
# reference's top-two score gap is at least gap_bound(k) at EVERY pixel
VOTE_CASES = {
    (2, 2): (0, True), (2, 19): (2, False), (2, 64): (2, True),
    (5, 2): (0, False), (5, 19): (0, True), (5, 64): (0, False),
    (16, 2): (0, True), (16, 19): (0, False), (16, 64): (6, True),
}


def make_views(k, c, n, seed, sizes=VIEW_SIZES):
    """k views of (n, c, h_i, w_i) float32 logits with |v| <= 8, sizes and flips mixed -> (logits_list, flips)"""
    rng = np.random.RandomState(seed)
    logits, flips = [], []
    for i in range(k):
        h, w = sizes[(i + seed) % len(sizes)]
        logits.append(np.clip(rng.standard_normal((n, c, h, w)) * 3.0, -8.0, 8.0).astype(np.float32))
        flips.append(bool((i // 2 + i) % 2))
    return logits, flips


def make_labels(shape, c, seed, dtype=np.uint8):
    rng = np.random.RandomState(seed + 1000)
    lab = rng.randint(0, c, size=shape)
    lab[rng.uniform(size=shape) < 0.1] = 255
    return lab.astype(dtype)


@functools.lru_cache(maxsize=None)
def vote_case(k, c):
    """-> dict(logits, flips, align, labels, pred, gap, cm), computed once"""
    seed, align = VOTE_CASES[(k, c)]
    n, H, W = OUT
    logits, flips = make_views(k, c, n, seed)
    _, pred, gap = vote(logits, flips, (H, W), align)
    labels = make_labels((n, H, W), c, seed)
    return dict(logits=logits, flips=flips, align=align, labels=labels, pred=pred, gap=gap, cm=confusion(labels, pred, c))


RESIZE_CASES = [((2, 3, 33, 47), (17, 24), False), ((2, 3, 33, 47), (50, 71), False), ((2, 3, 33, 47), (33, 47), True),
                ((1, 3, 1, 1), (4, 4), False)]


def resize_input(shape, seed=0):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
