"""
Test helper: the fp64 restatement, in plain numpy, of the class-threshold consistency (csrc/cthresh.hip; definition in
include/cutmixseg.h and DESIGN 8) -- the loss of tests/_loss_refs.py with the pass bit conf >= thr[k*] in the place of
conf >= tau, the integer statistics of a call, and the update arithmetic -- plus the cases, threshold vectors, margins and bounds the
CPU and GPU tests share. Upsample, per-pixel formulas, paste bits, inputs and the bound construction are _loss_refs'; nothing here
imports the product.

Statistics bound. The device rounds rint(v * 2^24) of an fp32 v; the restatement of an fp64 v. Per valid pixel the two integers
differ by at most 1 (two roundings to an integer, half each) + 2^24 |v32 - v64|, and |v32 - v64| <= K u32 a (1 + L) by the
construction of _loss_refs: a = the absolute-value form of v (v itself: a softmax probability is a quotient of positive terms), L the
largest absolute upsampled logit of the pixel, K = MARGIN * KAPPA_Q. KAPPA_Q is measured the way _loss_refs measures KAPPA: these
formulas in numpy fp32 (four-tap upsample included) against fp64 on these inputs; tests/test_cthresh_cpu.py asserts that no case
exceeds the constant. It is not tuned on the device.
"""
import math

import numpy as np

import _loss_refs as L

U32 = L.U32
MARGIN = L.MARGIN
RESEED = {'sy1': 1, 'span42': 1}
KAPPA_Q = 4.5           # largest measured |q32 - q64| / (u32 q (1 + L)) over the cases below, rounded up (the CPU test prints them)
GAP = 1e-4              # the two largest upsampled teacher logits of a pixel differ by at least this (as tests/_cps_refs.py)
CONF = 1e-5             # |conf - thr[k*]| is at least this
FIX = 2.0 ** 24
RAMP, WEIGHT = L.RAMP, L.WEIGHT

# (geometry of _loss_refs.GEOS, mask mode, loss, per-pixel confidence, mask given as): what each reaches is in the issue's table --
#   span42 C = 2 | sy1 C = 5 | tab2c19 C = 19, table loop, two tile columns | ratio2s C = 21, opt-in LDS | cmp33 run-time class count,
#   partial tiles | near1 direct-gather forward | identc3 identity forward and backward, no fused launch | one 1 x 1 logits |
#   identc5 the identity kernels with a compile-time class count (appended: tests index this list)
CASES = [
    ('span42', 'mix', 'var', False, 'ranges'),
    ('sy1', 'cut', 'kld', True, 'mask'),
    ('tab2c19', 'mix', 'var', True, 'ranges'),
    ('ratio2s', 'mix', 'bce', False, 'mask'),
    ('ratio2s', 'cut', 'logits_smoothl1', True, 'ranges'),
    ('cmp33', 'cut', 'logits_var', False, 'ranges'),
    ('cmp33', 'mix', 'kld', True, 'mask'),
    ('near1', 'mix', 'var', False, 'ranges'),
    ('identc3', 'mix', 'kld', True, 'ranges'),
    ('identc3', 'cut', 'var', False, 'mask'),
    ('one', 'cut', 'bce', True, 'ranges'),
    ('identc5', 'mix', 'var', True, 'ranges'),          # the identity kernels with a compile-time class count, the per-pixel gate on
]
REFUSED = ('toobig', 'mix', 'var', False, 'ranges')
VECTORS = ('ascending', 'one', 'floor')
# what tile_facts must say of a geometry (checked by the CPU test, as test_loss_refs_cpu.py checks GEOS)
ROUTES = {
    'span42': dict(forward='tiled', backward='tiled', fused=True), 'sy1': dict(forward='tiled', backward='tiled', fused=True),
    'tab2c19': dict(forward='tiled', backward='tiled', fused=True, tiles_x=2, table_all=True),
    'ratio2s': dict(forward='tiled_optin', backward='tiled_optin', fused=True),
    'cmp33': dict(forward='tiled', backward='tiled', fused=True), 'near1': dict(forward='direct', backward='tiled_optin', fused=True),
    'identc3': dict(forward='identity', backward='identity', fused=False),
    'identc5': dict(forward='identity', backward='identity', fused=False), 'one': dict(forward='tiled', backward='tiled', fused=True),
    'toobig': dict(forward='direct', backward='error', fused=False),
}


def case_id(case):
    return '-'.join(str(v) for v in case)


def geometry(name):
    return L.GEOS[name][:7]


def inputs(case):
    """_loss_refs.case_inputs, with the boxes as a materialised float mask where the case says so"""
    name, mode, fn, pp, given = case
    N, C, h, w, H, W, ac = geometry(name)
    i = dict(L.case_inputs(name, mode))
    if name in RESEED:
        # _loss_refs' recipe from another seed: with its own seed the fp64 reference has a pixel whose two largest teacher logits lie
        # closer than GAP (5.7e-5 for sy1) or a confidence within CONF of the 1.0 entry (9.3e-6 for span42, two classes); RESEED
        # holds the first seed from 1 upwards at which every pixel keeps both margins under all three vectors
        N, C = i['ls'].shape[:2]
        rng = np.random.RandomState(RESEED[name])
        i['ls'] = (rng.randn(*i['ls'].shape) * 2).astype(np.float32)
        i['l0'] = (rng.randn(*i['ls'].shape) * 3).astype(np.float32)
        l1 = (rng.randn(*i['ls'].shape) * 3).astype(np.float32)
        i['l1'] = l1 if mode == 'mix' else None
    if given == 'mask':
        i['mask'] = L.box_mask(i['ranges'], H, W, True).astype(np.float32)[:, None]
        i['ranges'] = None
    else:
        i['mask'] = None
    return i


# ------------------------------------------------------------------------------------------------------------ the teacher row
def teacher_rows(i, H, W, ac, mode, dtype=np.float64):
    """-> dict: up_t (N, C, H, W) pasted upsampled teacher logits, m paste bits, valid (statistics), um (loss weight), and in `dtype`
    conf, q (N, C, H, W), kstar, gap (top-two logit gap), Lt (largest |logit| of the teacher row, absolute-value form)"""
    N = i['l0'].shape[0]
    m = L.paste_bits(N, H, W, i['ranges'], i['mask'], True)
    one = np.ones((N, H, W))
    u0 = one if i['um0'] is None else np.asarray(i['um0'], dtype=np.float64).reshape(N, H, W)
    u1 = one if i.get('um1') is None else np.asarray(i['um1'], dtype=np.float64).reshape(N, H, W)
    up = (lambda x: L.upsample(x, H, W, ac)) if dtype is np.float64 else (lambda x: L.upsample_taps(x, H, W, ac, dtype))
    aup = lambda x: L.upsample(np.abs(np.asarray(x, dtype=np.float64)), H, W, ac)
    if mode == 'mix':
        up_t = np.where(m[:, None], up(i['l1']), up(i['l0']))
        a_t = np.where(m[:, None], aup(i['l1']), aup(i['l0']))
        um, valid = np.where(m, u1, u0), np.where(m, u1, u0) >= 0.5
    else:
        up_t, a_t = up(i['l0']), aup(i['l0'])
        um, valid = np.where(m, u0, 0.0), u0 >= 0.5           # valid: um0 whatever the mask bit
    q, mx, z = L._softmax(np.asarray(up_t, dtype=dtype), dtype)
    conf = (dtype(1) / z[:, 0]).astype(dtype)
    kstar = np.argmax(up_t == up_t.max(axis=1, keepdims=True), axis=1)        # the smallest index that attains the maximum
    if up_t.shape[1] > 1:
        top = np.sort(up_t, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(kstar.shape, np.inf)
    return dict(up_t=up_t, m=m, valid=valid, um=um, conf=conf, q=q, kstar=kstar, gap=gap, Lt=a_t.max(axis=1))


def table_of(rows, thr):
    """the integer table of one call: [n_valid | S_conf | S_c | N_pred | N_pass] as Python ints, and its bound per slot"""
    C = rows['q'].shape[1]
    v = rows['valid']
    thr64 = np.asarray(thr, dtype=np.float32).astype(np.float64)
    conf = rows['conf'].astype(np.float64)
    passed = conf >= thr64[rows['kstar']]
    fix = lambda x: np.rint(np.clip(x, 0.0, 1.0) * FIX).astype(np.int64)
    tab = [int(v.sum()), int(fix(conf)[v].sum())]
    tab += [int(fix(rows['q'][:, c].astype(np.float64))[v].sum()) for c in range(C)]
    tab += [int((v & (rows['kstar'] == c)).sum()) for c in range(C)]
    tab += [int((v & (rows['kstar'] == c) & passed).sum()) for c in range(C)]
    K = MARGIN * KAPPA_Q
    per = lambda a: float((1.0 + FIX * K * U32 * a * (1.0 + rows['Lt']))[v].sum())
    bound = [0.0, per(conf)] + [per(rows['q'][:, c].astype(np.float64)) for c in range(C)] + [0.0] * (2 * C)
    return tab, bound, passed


def kappa_q(i, H, W, ac, mode):
    """largest |fp32 - fp64| / (u32 v (1 + L)) of conf and q when the same formulas run in numpy fp32"""
    r64, r32 = teacher_rows(i, H, W, ac, mode), teacher_rows(i, H, W, ac, mode, np.float32)
    worst = 0.0
    for key in ('conf', 'q'):
        a, b = r64[key], r32[key].astype(np.float64)
        Lt = r64['Lt'] if a.ndim == 3 else r64['Lt'][:, None]
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(a == b, 0.0, np.abs(a - b) / (U32 * a * (1.0 + Lt)))
        worst = max(worst, float(r.max()))
    return worst


# ------------------------------------------------------------------------------------------------------------ threshold vectors
def _place(values, target, window=40, above=-1.0):
    """an fp32 threshold near `target` (and beyond `above`) in the middle of the widest gap between neighbouring confidences around it"""
    v = np.unique(values)
    v = np.concatenate([[0.8 * v[0]], v, [min(1.0, v[-1] + 0.1)]])      # room below the smallest and above the largest value
    target = max(target, above)
    j = int(np.clip(np.searchsorted(v, target), 1, len(v) - 1))
    ks = np.arange(1, len(v))
    ks = ks[0.5 * (v[ks - 1] + v[ks]) > above + 1e-3]
    if len(ks) == 0:
        return np.float32(min(1.0, above + 0.01))
    near = ks[np.abs(ks - j) <= window]
    ks = near if len(near) else ks[:window]
    k = int(ks[np.argmax(v[ks] - v[ks - 1])])
    return np.float32(0.5 * (v[k - 1] + v[k]))


def vectors(rows):
    """name -> fp32 thr (C,): about half the pixels pass, and no single scalar threshold gives the same bits.
      ascending  the 30 % ... 70 % quantiles of all confidences, rising with the class index
      one        per-class medians, one class at 1.0 (it never passes: no confidence is exactly 1 here) -- of the classes the
                 teacher predicts, the one whose largest confidence lies furthest below 1, so that the margin holds
      floor      per-class medians, the same class at 0.0 (the floor: it always passes)"""
    C = rows['q'].shape[1]
    conf, k = rows['conf'].astype(np.float64), rows['kstar']
    of = lambda c: conf[k == c] if (k == c).any() else conf.ravel()
    big = min((c for c in range(C) if (k == c).any()), key=lambda c: conf[k == c].max())
    asc = []
    for c in range(C):
        # (placed among ALL confidences: a class with few pixels has gaps so wide that a rising sequence would run away)
        asc.append(_place(conf.ravel(), np.quantile(conf, 0.3 + 0.4 * c / max(C - 1, 1)), above=float(asc[-1]) if asc else -1.0))
    asc = np.array(asc, dtype=np.float32)
    med = np.array([_place(of(c), np.median(of(c))) for c in range(C)], dtype=np.float32)
    one, flo = med.copy(), med.copy()
    one[big], flo[big] = 1.0, 0.0
    return dict(ascending=asc, one=one, floor=flo)


# ------------------------------------------------------------------------------------------------------------ the loss
def consistency(i, H, W, ac, mode, fn, thr, per_pixel, ramp=1.0, weight=1.0):
    """_loss_refs.consistency with conf >= thr[k*] in the place of conf >= tau (always on) -> the same dict (so grad_bound and
    scalar_bound of _loss_refs apply with the reference's own factors), plus table / table_bound / conf_margin / gap / passed."""
    l_stu = np.asarray(i['ls'], dtype=np.float64)
    N, C, h, w = l_stu.shape
    rows = teacher_rows(i, H, W, ac, mode)
    up_s, a_s = L.upsample(l_stu, H, W, ac), L.upsample(np.abs(l_stu), H, W, ac)
    a_t = L.upsample(np.abs(np.asarray(i['l0'], dtype=np.float64)), H, W, ac)
    if mode == 'mix':
        a_t = np.where(rows['m'][:, None], L.upsample(np.abs(np.asarray(i['l1'], dtype=np.float64)), H, W, ac), a_t)
    t = L.pixel_terms(up_s, rows['up_t'], fn, np.float64, a_s, a_t)
    tab, tbound, passed = table_of(rows, thr)
    um = rows['um']
    P = float(N * H * W)
    cf = passed.astype(np.float64)
    rate = cf.sum() / P
    loss = t['loss']
    if per_pixel:
        pm, gs = um * cf, 1.0 / P
        closs = (loss * pm).sum() / P
    else:
        pm, gs = um, rate / P
        closs = rate * ((loss * um).sum() / P)
    closs *= ramp
    gscale = gs * ramp * weight
    f = gscale * pm
    fg = f[:, None] * t['g']
    fa = np.abs(f)[:, None] * t['a'] * (1.0 + t['L'])[:, None]
    _, _, d = L.matrices(h, w, H, W, ac)
    thr64 = np.asarray(thr, dtype=np.float32).astype(np.float64)
    return dict(scalars=(closs, rate, gscale, closs * weight), grad=L.adjoint(fg, h, w, ac), fg=fg, fa=fa, d=d, conf=rows['conf'],
                lm=loss * pm, alm=np.abs(pm) * t['aloss'] * (1.0 + t['L']),
                value_scale=(rate if not per_pixel else 1.0) * ramp / P, P=P, h=h, w=w, ac=ac, fn=fn,
                table=tab, table_bound=tbound, passed=passed, kstar=rows['kstar'], valid=rows['valid'],
                conf_margin=float(np.abs(rows['conf'] - thr64[rows['kstar']]).min()), gap=float(rows['gap'].min()))


_cache = {}


def rows_of(case):
    key = ('rows',) + tuple(case[:2]) + (case[4],)
    if key not in _cache:
        N, C, h, w, H, W, ac = geometry(case[0])
        _cache[key] = teacher_rows(inputs(case), H, W, ac, case[1])
    return _cache[key]


def thr_of(case, vec):
    return vectors(rows_of(case))[vec]


def reference(case, vec):
    """what the tests keep of one (case, vector): computed once per session and left unchanged"""
    key = ('ref', tuple(case), vec)
    if key not in _cache:
        name, mode, fn, pp, given = case
        N, C, h, w, H, W, ac = geometry(name)
        thr = thr_of(case, vec)
        r = consistency(inputs(case), H, W, ac, mode, fn, thr, pp, RAMP, WEIGHT)
        _cache[key] = dict(thr=thr, scalars=r['scalars'], grad=r['grad'], bound=L.grad_bound(r), sbound=L.scalar_bound(r), P=r['P'],
                           table=r['table'], table_bound=r['table_bound'], conf_margin=r['conf_margin'], gap=r['gap'],
                           pass_share=float(r['passed'].mean()),
                           scalar_like=bool(r['conf'][r['passed']].min() > r['conf'][~r['passed']].max())
                           if r['passed'].any() and (~r['passed']).any() else True)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------ the update
def update(state, thr, table, epoch, C, adaptive, lam, floor, ceil):
    """cms_cthresh_update in Python floats (fp64), every product and sum rounded once: -> (state, thr fp32, table, epoch), new lists"""
    state, thr, table, epoch = list(state), [np.float32(v) for v in thr], [int(v) for v in table], [int(v) for v in epoch]
    n_valid = table[0]
    if adaptive and n_valid > 0:
        den = 16777216.0 * float(n_valid)
        one_m = 1.0 - lam
        state[0] = lam * state[0] + one_m * (float(table[1]) / den)
        for c in range(C):
            state[1 + c] = lam * state[1 + c] + one_m * (float(table[2 + c]) / den)
        pmax = max(state[1:1 + C])
        for c in range(C):
            thr[c] = np.float32(min(ceil, max(floor, state[0] * state[1 + c] / pmax)))
    epoch[0] += n_valid
    for c in range(C):
        epoch[1 + c] += table[2 + C + c]
        epoch[1 + C + c] += table[2 + 2 * C + c]
    return state, thr, [0] * (2 + 3 * C), epoch


def initial(C, floor=0.0, ceil=0.97):
    t0 = 1.0 / C
    return [t0] * (1 + C), [np.float32(min(ceil, max(floor, t0 * t0 / t0)))] * C


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))
