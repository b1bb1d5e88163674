"""Test helper: the fp64 restatement, in plain numpy, of sliding-window evaluation (csrc/window.hip; include/cutmixseg.h states the
definition) on _tta_refs.upsample / softmax, the cases the CPU and GPU tests share, and the driver of the host-check program
(tests/hostcheck_window). Nothing here imports the product.

The restatement does not use the closed form the kernel uses: it pastes every window's probabilities into a view-sized canvas beside a
count map, divides, and reads the view at every canvas pixel -- the tensor formulation the kernel replaces.

Exact comparison of predictions needs a condition on the inputs, not a tolerance: every case's logits are drawn (its seed searched on
the CPU, tests/test_window_cpu.py::test_case_margins re-checks it) so that the reference decides EVERY pixel by more than GAP_BOUND."""
import functools
import struct

import numpy as np

import _hostcheck
import _tta_refs as T

# Twice the largest |fp32 - fp64| error of a pixel's score over every case below, rounded up to two digits. The fp32 scores are the
# host-check program's (csrc/window_math.hpp compiled for the host: `pytest tests/test_window_hostcheck.py -s -k restatement` prints
# the figure per case). 2026-10-21: the largest is 5.92e-6 in single_k1_c21, whose scores are interpolated LOGITS of up to 13 in
# magnitude (one view of one window is scored on its logits, as cms_tta_vote scores it); among the cases whose scores are sums of
# probabilities it is 2.65e-6 (mixed_c21_k5_a0: five views, the (5, 7) logits read under align_corners=False).
GAP_BOUND = 1.2e-5


# ------------------------------------------------------------------------------------------------------------------ the grid
def axis_grid(view, window, stride):
    """one axis -> (effective window, [origins])"""
    e = min(window, view)
    g = 1 if view <= window else -(-(view - window) // stride) + 1
    return e, [min(j * stride, view - e) for j in range(g)]


def view_coord(canvas, view):
    """the view row of every canvas row: min(view - 1, ((2 y + 1) view) // (2 canvas))"""
    y = np.arange(canvas, dtype=np.int64)
    return np.minimum(view - 1, ((2 * y + 1) * view) // (2 * canvas))


def cover_count(view_size, window, stride):
    """(Hv, Wv) int: how many windows hold every pixel of the view, by pasting"""
    (eh, ys), (ew, xs) = axis_grid(view_size[0], window[0], stride[0]), axis_grid(view_size[1], window[1], stride[1])
    cnt = np.zeros(view_size, dtype=np.int64)
    for y1 in ys:
        for x1 in xs:
            cnt[y1:y1 + eh, x1:x1 + ew] += 1
    return cnt


def max_cover_axis(view, window, stride):
    """the most windows of one axis that can hold a coordinate: ceil(e / s) regular ones, one more when the flush last window is off
    the regular grid, never more than there are"""
    e, origins = axis_grid(view, window, stride)
    g = len(origins)
    return min(g, -(-e // stride) + (1 if g > 1 and (view - e) % stride else 0))


# ------------------------------------------------------------------------------------------------------------------ the definition
def stitch(logits_list, flips, view_sizes, window, stride, size, align_corners):
    """-> (score (n,c,H,W) fp64, pred (n,H,W) uint8, gap (n,H,W): best score minus runner-up; inf for one class)"""
    H, W = size
    grids = [(axis_grid(hv, window[0], stride[0]), axis_grid(wv, window[1], stride[1])) for hv, wv in view_sizes]
    if all(len(ys) * len(xs) == 1 for (_, ys), (_, xs) in grids):
        return T.vote(logits_list, flips, size, align_corners)              # the call IS the vote over whole views
    score = 0.0
    for l, flip, (hv, wv), ((eh, ys), (ew, xs)) in zip(logits_list, flips, view_sizes, grids):
        l = np.asarray(l, dtype=np.float64)
        g = len(ys) * len(xs)
        if g == 1:
            score = score + T.softmax(T.upsample(l, size, align_corners, flip), 1)
            continue
        n = l.shape[0] // g
        acc = np.zeros((n, l.shape[1], hv, wv))
        for j, y1 in enumerate(ys):
            for i, x1 in enumerate(xs):
                items = (np.arange(n) * len(ys) + j) * len(xs) + i
                acc[:, :, y1:y1 + eh, x1:x1 + ew] += T.softmax(T.upsample(l[items], (eh, ew), align_corners), 1)
        mean = acc / cover_count((hv, wv), window, stride)
        ry, rx = view_coord(H, hv), view_coord(W, wv)
        if flip:
            rx = wv - 1 - rx
        score = score + mean[:, :, ry[:, None], rx[None, :]]
    pred = score.argmax(axis=1)
    if score.shape[1] > 1:
        top = np.sort(score, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(pred.shape, np.inf)
    return score, pred.astype(np.uint8), gap


# ------------------------------------------------------------------------------------------------------------------ shared cases
OUT = (2, 37, 53)                                           # n, H, W of every case
WIN, STRIDE = (16, 24), (11, 16)                            # on the canvas: 3 x 3 windows, overlaps of 5 / 6 rows and 8 / 11 columns
CANVAS, HALF, SMALL, LARGE = (37, 53), (19, 27), (12, 20), (60, 80)

# name -> c, align, window, stride, views [(view size, flip, logits size | None for the window's own size)], int64 labels, seed
CASES = {
    'w3x3_c21_k1_a1_ident': dict(c=21, align=True, window=WIN, stride=STRIDE, views=[(CANVAS, False, None)], seed=0),
    'w3x3_c2_k1_a0_low': dict(c=2, align=False, window=WIN, stride=STRIDE, views=[(CANVAS, False, (5, 7))], seed=0),
    'w3x3_c64_k2_a0_flip': dict(c=64, align=False, window=WIN, stride=STRIDE, views=[(CANVAS, False, (5, 7)), (CANVAS, True, (5, 7))], seed=0),
    'nooverlap_c21_k1_a1': dict(c=21, align=True, window=WIN, stride=WIN, views=[(CANVAS, True, (4, 6))], seed=2),
    'dense_c21_k1_a0_i64': dict(c=21, align=False, window=WIN, stride=(4, 6), views=[(CANVAS, False, None)], i64=True, seed=41),
    'dense_c2_k2_a1': dict(c=2, align=True, window=WIN, stride=(4, 6), views=[(CANVAS, True, (5, 7)), (HALF, False, None)], seed=0),
    'half_c21_k2_a1': dict(c=21, align=True, window=WIN, stride=STRIDE, views=[(CANVAS, False, (5, 7)), (HALF, True, (5, 7))], seed=4),
    'large_c21_k2_a0': dict(c=21, align=False, window=WIN, stride=STRIDE, views=[(LARGE, True, (5, 7)), (CANVAS, False, None)], seed=0),
    'mixed_c21_k5_a0': dict(c=21, align=False, window=WIN, stride=STRIDE,
                            views=[(CANVAS, False, (5, 7)), (CANVAS, True, (5, 7)), (HALF, False, None), (SMALL, True, (5, 7)),
                                   (SMALL, False, None)], seed=0),
    'mixed_c64_k5_a1': dict(c=64, align=True, window=WIN, stride=STRIDE,
                            views=[(SMALL, True, None), (LARGE, False, (5, 7)), (CANVAS, True, None), (HALF, True, (5, 7)),
                                   (SMALL, False, (5, 7))], i64=True, seed=0),
    'small_first_c2_k2_a0_i64': dict(c=2, align=False, window=WIN, stride=STRIDE, views=[(SMALL, False, (5, 7)), (CANVAS, True, None)],
                                     i64=True, seed=1),
    'one_axis_c21_k2_a1': dict(c=21, align=True, window=WIN, stride=STRIDE, views=[((12, 53), False, (5, 7)), ((37, 20), True, None)],
                               seed=4),
    # no view has more than one window: the call is cms_tta_vote
    'single_k1_c21': dict(c=21, align=False, window=WIN, stride=STRIDE, views=[(SMALL, True, (5, 7))], seed=0),
    'single_k1_c21_ident': dict(c=21, align=True, window=(40, 56), stride=(27, 38), views=[(CANVAS, False, None)], seed=0),
    'single_k2_c19': dict(c=19, align=True, window=WIN, stride=STRIDE, views=[(SMALL, False, (5, 7)), (SMALL, True, None)], seed=1),
}


def layout(name):
    """-> per view dict(Hv, Wv, flip, gy, gx, eh, ew, hl, wl) of a case"""
    spec = CASES[name]
    out = []
    for (hv, wv), flip, low in spec['views']:
        (eh, ys), (ew, xs) = axis_grid(hv, spec['window'][0], spec['stride'][0]), axis_grid(wv, spec['window'][1], spec['stride'][1])
        hl, wl = low if low is not None else (eh, ew)
        out.append(dict(Hv=hv, Wv=wv, flip=bool(flip), gy=len(ys), gx=len(xs), eh=eh, ew=ew, hl=hl, wl=wl))
    return out


def make_logits(name, n, seed):
    """the window logits of every view of a case: float32, N(0, 3^2). Not clipped: where a window's logits have its own size and no
    other window holds the pixel, two clipped classes would tie exactly"""
    rng = np.random.RandomState(seed)
    c = CASES[name]['c']
    return [(rng.standard_normal((n * v['gy'] * v['gx'], c, v['hl'], v['wl'])) * 3.0).astype(np.float32) for v in layout(name)]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(c, align, window, stride, logits, flips, view_sizes, layout, labels, score, pred, gap, cm), computed once"""
    spec = CASES[name]
    n, H, W = OUT
    lay = layout(name)
    logits = make_logits(name, n, spec['seed'])
    flips, sizes = [v['flip'] for v in lay], [(v['Hv'], v['Wv']) for v in lay]
    score, pred, gap = stitch(logits, flips, sizes, spec['window'], spec['stride'], (H, W), spec['align'])
    labels = T.make_labels((n, H, W), spec['c'], spec['seed'], np.int64 if spec.get('i64') else np.uint8)
    return dict(c=spec['c'], align=spec['align'], window=spec['window'], stride=spec['stride'], logits=logits, flips=flips,
                view_sizes=sizes, layout=lay, labels=labels, score=score, pred=pred, gap=gap,
                cm=T.confusion(labels, pred, spec['c']), all_single=all(v['gy'] * v['gx'] == 1 for v in lay))


# ------------------------------------------------------------------------------------------------------------------ host check
NULLS = dict(labels=1, cm=2, pred_out=4, logits=8)
VIEW_FIELDS = ('hl', 'wl', 'Hv', 'Wv', 'gy', 'gx', 'eh', 'ew', 'sh', 'sw', 'flip')


def hostcheck_run(exe, cs, expect_code=0, null=(), views=None, **over):
    """one vote request through the host driver -> dict(cm, claims, pred, score), or None when it ends with `expect_code` != 0.
    `over`: header fields (n, c, H, W, k, align, label_dtype, ignore, wh, ww) sent as they are; `views`: {view index: {field: value}}
    overrides of the per-view table."""
    n, H, W = OUT
    c = cs['c']
    head = dict(n=n, c=c, H=H, W=W, k=len(cs['logits']), align=int(cs['align']), label_dtype=int(cs['labels'].dtype == np.int64),
                ignore=255, wh=cs['window'][0], ww=cs['window'][1])
    head.update(over)
    table = []
    for i, v in enumerate(cs['layout']):
        row = dict(v, sh=cs['stride'][0], sw=cs['stride'][1], flip=int(v['flip']))
        row.update((views or {}).get(i, {}))
        table.append(row)
    header = struct.pack('<12i', 0, head['n'], head['c'], head['H'], head['W'], head['k'], head['align'], head['label_dtype'],
                         head['ignore'], head['wh'], head['ww'], sum(NULLS[x] for x in null))
    for row in table:
        header += struct.pack('<11i', *[row[name] for name in VIEW_FIELDS])
    blocks = []
    for t in cs['logits']:
        blocks += [(t.size, '<i8'), (t, np.float32)]
    raw = _hostcheck.run(exe, header, blocks + [(cs['labels'], None)], expect_code)
    if raw is None:
        return None
    out = _hostcheck.split(raw, [('cm', np.int64, (c, c)), ('claims', np.int64, (1,)), ('pred', np.uint8, (n, H, W)),
                                 ('score', np.float32, (n, c, H, W))])
    return dict(out, claims=int(out['claims'][0]))


def hostcheck_crop(exe, x, view_size, flip, window, stride, expect_code=0):
    """one crop request -> (n * G, c, eh, ew) float32"""
    n, c, H, W = x.shape
    header = struct.pack('<12i', 1, n, c, H, W, view_size[0], view_size[1], int(flip), window[0], window[1], stride[0], stride[1])
    raw = _hostcheck.run(exe, header, [(x, np.float32)], expect_code)
    if raw is None:
        return None
    (eh, ys), (ew, xs) = axis_grid(view_size[0], window[0], stride[0]), axis_grid(view_size[1], window[1], stride[1])
    return _hostcheck.split(raw, [('crops', np.float32, (n * len(ys) * len(xs), c, eh, ew))])['crops']
