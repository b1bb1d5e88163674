"""Test helper: the fp64 restatement, in plain numpy, of the calibration launch (csrc/calib.hip; include/cutmixseg.h and DESIGN 8 state
the definition) on _tta_refs.upsample / softmax, the cases the CPU and GPU tests share, the acceptance rule, and the driver of the
host-check program (tests/hostcheck_calib). Nothing here imports the product.

A pixel's cell (predicted class, confidence bin) is decided in fp32 by the kernel and in fp64 here, so a pixel whose fp64 confidence
lies within 4 * B_CONF of an interior edge, or whose two best classes are closer than _tta_refs.gap_bound(k) / k, may fall into one of
two cells: it is AMBIGUOUS. The restatement returns the SURE tables (from the other pixels) and, per cell, how many ambiguous pixels MAY
fall into it; a result is accepted when sure <= got <= sure + maybe in every cell. That ambiguous pixels are at most 1 % of the scored
pixels is a condition on every case (tests/test_calib_cpu.py asserts it), not a measurement."""
import functools
import struct

import numpy as np

import _hostcheck
import _tta_refs as T

FLT_MIN = float(np.finfo(np.float32).tiny)
CONF_SCALE, BRIER_SCALE, NLL_SCALE, NLL_CAP = 2.0 ** 24, 2.0 ** 24, 2.0 ** 20, 88.0

# Per-pixel bounds on |fp32 - fp64| of the confidence, the squared error and the NLL: twice the host-check program's largest error over
# every case below, rounded up to two digits (`pytest tests/test_calib_hostcheck.py -s -k restatement` prints the three figures per
# case; 2026-10-20: conf 8.21e-6, squared error 1.93e-5, nll 1.05e-4, all three in k2_c19_T0.5, whose (60, 80) view is read under
# align_corners=False: pixel_math.hpp's bilin_tap places the sample in fp32, a few 1e-6 of a pixel off, between neighbouring logits
# that differ by up to 32 at T = 0.5). The kernel's own per-pixel error cannot be observed -- only sums leave it -- so no MI355X
# figure enters: the host figure alone, as DESIGN 8 records. What the GPU test does measure is the kernel's MEAN error per table,
# printed per case by `pytest tests/test_gpu_calib.py -s -k restatement`.
B_CONF = 1.7e-5
B_BRIER = 3.9e-5
B_NLL = 2.2e-4
MAX_AMBIGUOUS = 0.01
DEFAULT_THRESHOLDS = (0.5, 0.9, 0.95, 0.97, 0.99)


# ------------------------------------------------------------------------------------------------------------------ the partition
def make_edges(n_bins, thresholds):
    """the sorted union of i / n_bins and the thresholds, built in fp64, cast to fp32, duplicates merged -> float32 (nb - 1,)"""
    eq = (np.arange(1, n_bins, dtype=np.float64) / n_bins).astype(np.float32)
    return np.unique(np.concatenate([eq, np.asarray(thresholds, dtype=np.float64).astype(np.float32)]))


def bin_of(conf, edges):
    """#{j: edge_j <= conf}"""
    return np.searchsorted(np.asarray(edges, dtype=np.float64), conf, side='right')


# ------------------------------------------------------------------------------------------------------------------ the definition
def pixels(logits_list, flips, size, align_corners, temps):
    """-> dict(ups: the upsampled logits per view, inv: 1 / T per temperature, pbars: the mean distribution per temperature, and at
    temps[0] pred, conf, gap (the top-two gap of the mean distribution) and second (the runner-up class))"""
    k = len(logits_list)
    ups = [T.upsample(l, size, align_corners, f) for l, f in zip(logits_list, flips)]
    inv = [float(np.float32(1.0) / np.float32(t)) for t in temps]                 # 1 / T, rounded once to fp32
    pbars = [sum(T.softmax(u * it, 1) for u in ups) / k for it in inv]
    pbar = pbars[0]
    pred = (ups[0] if k == 1 else pbar).argmax(axis=1)                              # one view: the argmax of the logits themselves
    conf = np.minimum(np.take_along_axis(pbar, pred[:, None], 1)[:, 0], 1.0)
    if pbar.shape[1] > 1:
        top = np.sort(pbar, axis=1)
        gap, second = top[:, -1] - top[:, -2], np.argsort(pbar, axis=1)[:, -2]
    else:
        gap, second = np.full(pred.shape, np.inf), pred.copy()
    return dict(k=k, ups=ups, inv=inv, pbars=pbars, pred=pred, conf=conf, gap=gap, second=second)


def report(logits_list, flips, labels, size, align_corners, edges, temps, ignore=255):
    """The whole launch in fp64 -> dict of the sure tables, the maybe counts and the per-pixel values."""
    px = pixels(logits_list, flips, size, align_corners, temps)
    k, c = px['k'], logits_list[0].shape[1]
    nb, nt = len(edges) + 1, len(temps)
    lab = labels.astype(np.int64)
    valid = (lab != ignore) & (lab >= 0) & (lab < c)
    safe = np.where(valid, lab, 0)
    onehot = np.arange(c).reshape(1, c, 1, 1) == safe[:, None]
    brier = ((px['pbars'][0] - onehot) ** 2).sum(axis=1)
    nll = []
    for t in range(nt):
        if k == 1:
            u = px['ups'][0] * px['inv'][t]
            mx = u.max(axis=1)
            nll.append(-((np.take_along_axis(u, safe[:, None], 1)[:, 0] - mx) - np.log(np.exp(u - mx[:, None]).sum(axis=1))))
        else:
            nll.append(-np.log(np.maximum(np.take_along_axis(px['pbars'][t], safe[:, None], 1)[:, 0], FLT_MIN)))
    nll = np.stack(nll)
    conf, pred = px['conf'], px['pred']
    e64 = np.asarray(edges, dtype=np.float64)
    near = np.zeros(conf.shape, dtype=bool) if nb == 1 else np.abs(conf[..., None] - e64).min(axis=-1) <= 4 * B_CONF
    tie = px['gap'] < T.gap_bound(k) / k
    amb = valid & (near | tie)
    sure = valid & ~amb
    hist = np.zeros((c, nb, 3), dtype=np.int64)
    b = bin_of(conf, edges)
    fx = np.rint(np.clip(conf, 0.0, 1.0) * CONF_SCALE).astype(np.int64)
    np.add.at(hist[:, :, 0], (pred[sure], b[sure]), 1)
    np.add.at(hist[:, :, 1], (pred[sure], b[sure]), (pred[sure] == lab[sure]).astype(np.int64))
    np.add.at(hist[:, :, 2], (pred[sure], b[sure]), fx[sure])
    maybe = np.zeros((c, nb, 3), dtype=np.int64)
    for i in zip(*np.nonzero(amb)):
        classes = {int(pred[i])} | ({int(px['second'][i])} if tie[i] else set())
        bins = {int(b[i])}
        if near[i]:
            bins |= {int(bin_of(conf[i] - 4 * B_CONF, edges)), int(bin_of(conf[i] + 4 * B_CONF, edges))}
        for cc in classes:
            for bb in bins:
                maybe[cc, bb] += (1, int(cc == lab[i]), int(fx[i]) + 1)
    cm = T.confusion(np.where(valid, lab, 255).astype(np.int64), pred, c) if c <= 255 else None
    scores = np.zeros(2 + nt, dtype=np.int64)
    scores[0] = int(valid.sum())
    scores[1] = int(np.rint(np.clip(brier[valid], 0.0, 2.0) * BRIER_SCALE).sum())
    for t in range(nt):
        scores[2 + t] = int(np.rint(np.clip(nll[t][valid], 0.0, NLL_CAP) * NLL_SCALE).sum())
    return dict(hist=hist, maybe=maybe, scores=scores, cm=cm, pred=pred.astype(np.uint8), valid=valid, tie=tie, ambiguous=int(amb.sum()),
                edge_ambiguous=int((valid & near).sum()), tie_ambiguous=int((valid & tie).sum()), conf=conf, brier=brier, nll=nll,
                conf_fx_all=int(fx[valid].sum()))


def accept(got, ref):
    """The acceptance rule on a result dict(hist, scores, cm | None, pred | None) -> nothing; raises AssertionError"""
    hist, scores = np.asarray(got['hist'], dtype=np.int64), np.asarray(got['scores'], dtype=np.int64)
    sure, maybe = ref['hist'], ref['maybe']
    for j in (0, 1):
        assert (sure[:, :, j] <= hist[:, :, j]).all() and (hist[:, :, j] <= sure[:, :, j] + maybe[:, :, j]).all(), j
    n_scored = int(ref['scores'][0])
    assert int(hist[:, :, 0].sum()) == n_scored and int(scores[0]) == n_scored
    assert (hist[:, :, 1] <= hist[:, :, 0]).all()
    tol = hist[:, :, 0] * (B_CONF * CONF_SCALE + 1)
    assert (hist[:, :, 2] >= sure[:, :, 2] - tol).all() and (hist[:, :, 2] <= sure[:, :, 2] + maybe[:, :, 2] + tol).all()
    # all cells together: where a pixel fell does not matter (a tied pixel's two confidences differ by less than the gap bound)
    assert abs(int(hist[:, :, 2].sum()) - ref['conf_fx_all']) <= n_scored * (B_CONF * CONF_SCALE + 1)
    assert abs(int(scores[1]) - int(ref['scores'][1])) <= n_scored * (B_BRIER * BRIER_SCALE + 1)
    for t in range(len(scores) - 2):
        assert abs(int(scores[2 + t]) - int(ref['scores'][2 + t])) <= n_scored * (B_NLL * NLL_SCALE + 1), t
    firm = ~ref['tie']
    if got.get('pred') is not None:
        assert np.array_equal(np.asarray(got['pred'])[firm], ref['pred'][firm])
    if got.get('cm') is not None:
        cm = np.asarray(got['cm'], dtype=np.int64)
        loose = ref['valid'] & ref['tie']
        assert int(cm.sum()) == n_scored and np.abs(cm - ref['cm']).sum() <= 2 * int(loose.sum())
        if not loose.any():
            assert np.array_equal(cm, ref['cm'])


# ------------------------------------------------------------------------------------------------------------------ shared cases
OUT = T.OUT


def hot_views(k, c, n, seed, amp, sizes=T.VIEW_SIZES):
    """k views that AGREE: one coarse random field per class, sampled at every view's own grid (a flipped view holds the mirrored
    field) and scaled by `amp`, plus N(0, 1) noise -- so that the vote is confident over whole regions -> (logits_list, flips)"""
    rng = np.random.RandomState(seed + 77)
    field = rng.standard_normal((n, c, 4, 5))
    logits, flips = [], []
    for i in range(k):
        h, w = sizes[(i + seed) % len(sizes)]
        flip = bool((i // 2 + i) % 2)
        v = T.upsample(field, (h, w), True) * amp + rng.standard_normal((n, c, h, w))
        logits.append((v[..., ::-1] if flip else v).astype(np.float32).copy())
        flips.append(flip)
    return logits, flips


# name -> dict(k, c, seed, align, T (tuple, T[0] the histogram's), n_bins, thresholds, shape, dtype, hot (amplitude or None),
# ignore_all)
def _case(k, c, seed, align, temps=(1.0,), n_bins=15, thresholds=DEFAULT_THRESHOLDS, shape=OUT, dtype=np.uint8, hot=None,
          ignore_all=False):
    return dict(k=k, c=c, seed=seed, align=align, temps=tuple(temps), n_bins=n_bins, thresholds=tuple(thresholds), shape=shape,
                dtype=dtype, hot=hot, ignore_all=ignore_all)


# (k, C) -> (seed, align): one view of (5, 7) / identity size (37, 53) / (9, 13); the votes are _tta_refs.VOTE_CASES'
GRID = {(1, 2): (0, True), (1, 21): (2, False), (1, 19): (1, True), (2, 19): T.VOTE_CASES[(2, 19)], (5, 64): T.VOTE_CASES[(5, 64)],
        (16, 2): T.VOTE_CASES[(16, 2)]}
MORE_TEMPS = (0.5, 0.75, 1.25, 1.5, 2.0, 3.0, 4.0)
CASES = {}
for (_k, _c), (_seed, _align) in GRID.items():
    for _t in (1.0, 0.5, 2.0):
        CASES['k{}_c{}_T{:g}'.format(_k, _c, _t)] = _case(_k, _c, _seed, _align, (_t,))
CASES.update({
    'k2_c19_nt8': _case(2, 19, 2, False, (1.0,) + MORE_TEMPS),
    'k1_c19_nt8_i64': _case(1, 19, 1, False, (2.0,) + MORE_TEMPS, dtype=np.int64),
    'k1_c21_ident_align_i64': _case(1, 21, 2, True, dtype=np.int64),
    'k1_c2_noalign': _case(1, 2, 0, False),
    'k5_c64_i64': _case(5, 64, 0, True, dtype=np.int64),
    'lds_worst_k16_c64_nb48': _case(16, 64, 6, True, n_bins=43),
    'nb1_k2_c19': _case(2, 19, 2, False, n_bins=1, thresholds=()),
    'nb1_k1_c21': _case(1, 21, 2, False, n_bins=1, thresholds=()),
    'one_pixel_k1': _case(1, 21, 1, True, shape=(1, 1, 1)),
    'one_pixel_k2': _case(2, 19, 2, False, shape=(1, 1, 1)),
    'all_ignored_k1': _case(1, 19, 1, True, ignore_all=True),
    'all_ignored_k5': _case(5, 64, 0, False, ignore_all=True),
    # logits that reach the top bins, one per class count
    'hot_k1_c2': _case(1, 2, 0, True, hot=4.0),
    'hot_k1_c21': _case(1, 21, 2, False, hot=6.0),
    'hot_k2_c19': _case(2, 19, 2, False, hot=6.0),
    'hot_k5_c64': _case(5, 64, 0, False, hot=8.0, temps=(0.5,)),
})
HOT = sorted(n for n in CASES if CASES[n]['hot'])


def case_inputs(name):
    cs = CASES[name]
    n, H, W = cs['shape']
    if cs['hot']:
        logits, flips = hot_views(cs['k'], cs['c'], n, cs['seed'], cs['hot'])
    else:
        logits, flips = T.make_views(cs['k'], cs['c'], n, cs['seed'])
    labels = T.make_labels((n, H, W), cs['c'], cs['seed'], cs['dtype'])
    if cs['hot']:
        # labels that mostly agree with a confident network, so that the accuracy per bin is not chance
        pred = pixels(logits, flips, (H, W), cs['align'], (1.0,))['pred']
        keep = np.random.RandomState(cs['seed'] + 5).uniform(size=pred.shape) < 0.8
        labels = np.where((labels != 255) & keep, pred, labels).astype(cs['dtype'])
    if n * H * W == 1:
        labels = (labels % cs['c']).astype(cs['dtype'])              # the one pixel is scored
    if cs['ignore_all']:
        labels = np.full((n, H, W), 255, dtype=cs['dtype'])
    edges = make_edges(cs['n_bins'], cs['thresholds'])
    return dict(logits=logits, flips=flips, labels=labels, size=(H, W), align=cs['align'], edges=edges,
                temps=np.asarray(cs['temps'], dtype=np.float32), c=cs['c'], k=cs['k'], shape=(n, H, W))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, reference), computed once"""
    inp = case_inputs(name)
    return inp, report(inp['logits'], inp['flips'], inp['labels'], inp['size'], inp['align'], inp['edges'], inp['temps'])


# ------------------------------------------------------------------------------------------------------------------ host driver
NULLS = dict(labels=1, hist=2, scores=4, cm=8, pred_out=16, edges=32, temps=64)


def hostcheck_run(exe, inp, expect_code=0, null=(), **over):
    """one request through the host driver -> dict(hist, scores, cm, claims, pred, conf, brier, nll), or None when it ends with
    `expect_code` != 0. `over`: header fields (n, c, H, W, k, align, label_dtype, ignore, nb, nt) or `edges` / `temps` sent as they are."""
    n, c = inp['logits'][0].shape[:2]
    H, W = inp['size']
    edges = np.asarray(over.pop('edges', inp['edges']), dtype=np.float32)
    temps = np.asarray(over.pop('temps', inp['temps']), dtype=np.float32)
    head = dict(n=n, c=c, H=H, W=W, k=len(inp['logits']), align=int(inp['align']), label_dtype=int(inp['labels'].dtype == np.int64),
                ignore=255, nb=len(edges) + 1, nt=len(temps))
    head.update(over)
    header = struct.pack('<13i', head['n'], head['c'], head['H'], head['W'], head['k'], head['align'], head['label_dtype'],
                         head['ignore'], head['nb'], head['nt'], len(edges), len(temps), sum(NULLS[x] for x in null))
    header += edges.tobytes() + temps.tobytes()
    for t, fl in zip(inp['logits'], inp['flips']):
        header += struct.pack('<3i', t.shape[2], t.shape[3], int(fl))
    raw = _hostcheck.run(exe, header, [(t, np.float32) for t in inp['logits']] + [(inp['labels'], None)], expect_code)
    if raw is None:
        return None
    nb, nt = head['nb'], head['nt']
    return _hostcheck.split(raw, [('hist', np.int64, (c, nb, 3)), ('scores', np.int64, (2 + nt,)), ('cm', np.int64, (c, c)),
                                  ('claims', np.int64, (3,)), ('pred', np.uint8, (n, H, W)), ('conf', np.float32, (n, H, W)),
                                  ('brier', np.float32, (n, H, W)), ('nll', np.float32, (nt, n, H, W))])


def pixel_errors(got, ref):
    """-> the largest |fp32 - fp64| of (conf, squared error, nll) over the scored pixels that are not tied"""
    m = ref['valid'] & ~ref['tie']
    if not m.any():
        return 0.0, 0.0, 0.0
    return (float(np.abs(got['conf'][m] - ref['conf'][m]).max()), float(np.abs(got['brier'][m] - ref['brier'][m]).max()),
            float(np.abs(np.minimum(got['nll'][:, m], NLL_CAP) - np.minimum(ref['nll'][:, m], NLL_CAP)).max()))
