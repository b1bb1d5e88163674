"""
Plain references for the loss kernels (csrc/losses.hip): both losses restated from their DEFINITIONS in numpy fp64 -- dense bilinear
matrices, no tiles, no staging, no atomics -- plus the rounding-error bound the GPU tests assert with and a numpy restatement of the
host-side tile arithmetic that decides which kernel path a geometry takes (`tile_facts`). tests/test_loss_refs_cpu.py pins all of
it (committed fixtures, oracle/losses.py in fp64, the path of every geometry below); tests/test_gpu_loss_kernels.py holds the
kernels to it. Nothing here imports oracle/losses.py.

Bound. With U the dense fp32-weight upsampling matrix, f the per-pixel factor (ramp * weight * rate-or-1 / P * um *
confidence bit; weight / n_valid for the cross entropy), g_k the derivative of the pixel's loss with respect to its upsampled logit
k, the gradient with respect to the low-resolution logits is U^T (f g) and every element of a kernel's result is held to

    |got - ref| <= (d + 2) * u32 * U^T |f g|  +  U^T ( |f| * K * u32 * a_k * (1 + L) )

d = number of output pixels that touch the cell (the adjoint's addition chain), a_k = the formula of g_k with every subtraction
replaced by a sum of absolute values, L = the largest absolute upsampled logit of the pixel (the argument of an exponential is a
difference of two logits, so a relative error u32 of a logit is an absolute error up to 2 L u32 of the exponent), K = MARGIN *
KAPPA[loss]. KAPPA is MEASURED, not tuned on the device: the largest |fp32 - fp64| / (u32 * a_k * (1 + L)) when these same formulas
(four-tap upsample included) are evaluated in numpy fp32 on the tests' inputs (`pixel_terms(..., dtype=np.float32)`); the CPU test
asserts that no case exceeds the constant below. MARGIN = 4 pays for the device's expf / logf / reciprocal and its class-sum order,
which differ from numpy's by a few ulp each. Where the bound is not zero it carries (d + 2) * 2^-126 for results below fp32's normal
range (the logits of +-60 produce gradients of 1e-45). The scalars are held to the same construction over the pixel sum (`scalar_bound`).
"""
import math

import numpy as np

import _stream_refs as R

U32 = R.U32
TINY32 = 2.0 ** -126        # smallest normal fp32 number: below it a term loses its last bits or is flushed -- the relative model
                            # u32 * |x| of a rounding does not hold there, each of the d + 2 roundings may be off by up to this much
LOSS_FNS = ('var', 'logits_var', 'logits_smoothl1', 'bce', 'kld')
EPS = 1e-6
MARGIN = 4.0
# largest measured fp32-vs-fp64 error of the per-pixel GRADIENT / VALUE formulas in units of u32 * a * (1 + L), rounded up
# (test_loss_refs_cpu.py::test_kappa_of_every_case_is_below_the_constant prints the measured figures)
KAPPA = {'var': 4.5, 'logits_var': 1.0, 'logits_smoothl1': 1.0, 'bce': 3.0, 'kld': 3.5, 'ce': 4.5}
KAPPA_VALUE = {'var': 2.5, 'logits_var': 1.0, 'logits_smoothl1': 1.0, 'bce': 0.5, 'kld': 1.0, 'ce': 1.5}


# ------------------------------------------------------------------------------------------------------------ upsample / paste
def matrices(h, w, H, W, ac):
    My, cy = R.bilinear_matrix(h, H, ac, weight_dtype=np.float32)
    Mx, cx = R.bilinear_matrix(w, W, ac, weight_dtype=np.float32)
    return My, Mx, np.outer(cy, cx).astype(np.float64)


def upsample(x, H, W, ac):
    """(N, C, h, w) -> (N, C, H, W) in fp64 with the fp32 weights of the definition."""
    x = np.asarray(x, dtype=np.float64)
    My, Mx, _ = matrices(x.shape[2], x.shape[3], H, W, ac)
    return np.einsum('Yy,ncyX->ncYX', My, np.einsum('Xx,ncyx->ncyX', Mx, x, optimize=True), optimize=True)


def adjoint(g, h, w, ac):
    """U^T g: (N, C, H, W) -> (N, C, h, w)"""
    My, Mx, _ = matrices(h, w, g.shape[2], g.shape[3], ac)
    return np.einsum('Yy,ncYx->ncyx', My, np.einsum('Xx,ncYX->ncYx', Mx, g, optimize=True), optimize=True)


def upsample_taps(x, H, W, ac, dtype):
    """the same map as four taps per pixel, every operation rounded to `dtype` (the fp32 evaluation KAPPA is measured with)"""
    T = dtype
    x = np.asarray(x, dtype=T)
    y0, y1, wy0, wy1 = R.bilinear_taps(x.shape[2], H, ac, np.float32)
    x0, x1, wx0, wx1 = R.bilinear_taps(x.shape[3], W, ac, np.float32)
    wx0, wx1, wy0, wy1 = wx0.astype(T), wx1.astype(T), wy0.astype(T)[:, None], wy1.astype(T)[:, None]
    r0, r1 = x[:, :, y0, :], x[:, :, y1, :]
    a = (wx0 * r0[..., x0]).astype(T) + (wx1 * r0[..., x1]).astype(T)
    b = (wx0 * r1[..., x0]).astype(T) + (wx1 * r1[..., x1]).astype(T)
    return ((wy0 * a).astype(T) + (wy1 * b).astype(T)).astype(T)


def box_mask(ranges, H, W, invert):
    """ranges int (N, nb, 4) = [y0, y1, x0, x1) -> bool (N, H, W): XOR of the boxes; `invert` keeps the parity, else its complement"""
    ranges = np.asarray(ranges).reshape(len(ranges), -1, 4)
    yy, xx = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    par = np.zeros((ranges.shape[0], H, W), dtype=bool)
    for b in range(ranges.shape[1]):
        r = ranges[:, b, :].astype(np.int64)
        par ^= ((yy >= r[:, 0, None, None]) & (yy < r[:, 1, None, None]) & (xx >= r[:, 2, None, None]) & (xx < r[:, 3, None, None]))
    return par if invert else ~par


def paste_bits(N, H, W, ranges=None, mask=None, invert=True):
    if (ranges is None) == (mask is None):
        raise ValueError('give exactly one of ranges / mask')
    if mask is not None:
        return np.asarray(mask).reshape(N, H, W) >= 0.5
    return box_mask(ranges, H, W, invert)


# ------------------------------------------------------------------------------------------------------------ per-pixel formulas
def _softmax(l, T):
    mx = l.max(axis=1, keepdims=True)
    e = np.exp((l - mx).astype(T)).astype(T)
    z = e.sum(axis=1, keepdims=True, dtype=T)
    return (e / z).astype(T), mx, z


def pixel_terms(ls, lt, fn, dtype=np.float64, als=None, alt=None):
    """Upsampled student / teacher logits (N, C, H, W) -> dict of per-pixel quantities, every operation in `dtype`:
      loss (N, H, W)  the pixel's value (summed over classes, / sqrt(C) for the two logit losses),   aloss  its absolute-value form
      g (N, C, H, W)  d loss / d student logit k,                                                     a      its absolute-value form
      conf (N, H, W)  max softmax(teacher),   L (N, H, W)  the largest |logit| of the pixel (student and teacher).
    `als` / `alt`: the absolute-value form of the logits themselves, U |l| (an upsampled logit is a sum of four signed products: it
    can be small where its taps are not); |ls| / |lt| when not given."""
    T = dtype
    ls, lt = np.asarray(ls, dtype=T), np.asarray(lt, dtype=T)
    C = ls.shape[1]
    irc = T(1.0 / math.sqrt(C))
    eps = T(EPS)
    one = T(1)
    p, ms, zs = _softmax(ls, T)
    t, mt, zt = _softmax(lt, T)
    als = np.abs(ls) if als is None else np.asarray(als, dtype=T)
    alt = np.abs(lt) if alt is None else np.asarray(alt, dtype=T)
    out = dict(conf=t.max(axis=1), L=np.maximum(als.max(axis=1), alt.max(axis=1)))
    if fn == 'var':
        d, s = p - t, p + t
        dot = (2 * d * p).sum(axis=1, keepdims=True, dtype=T)
        adot = (2 * s * p).sum(axis=1, keepdims=True, dtype=T)
        out.update(loss=(d * d).sum(axis=1, dtype=T), aloss=(s * s).sum(axis=1, dtype=T), g=p * (2 * d - dot), a=p * (2 * s + adot))
    elif fn == 'logits_var':
        d, s = ls - lt, als + alt
        out.update(loss=(d * d).sum(axis=1, dtype=T) * irc, aloss=(s * s).sum(axis=1, dtype=T) * irc, g=2 * d * irc, a=2 * s * irc)
    elif fn == 'logits_smoothl1':
        d, s = ls - lt, als + alt
        ad = np.abs(d)
        small = ad < one
        out.update(loss=np.where(small, T(0.5) * d * d, ad - T(0.5)).sum(axis=1, dtype=T) * irc,
                   aloss=np.where(small, T(0.5) * s * s, s + T(0.5)).sum(axis=1, dtype=T) * irc,
                   g=np.where(small, d, np.sign(d)) * irc, a=np.where(small, s, one) * irc)
    elif fn == 'bce':
        q, aq = (one - p + eps).astype(T), (one + p + eps).astype(T)        # 1 - p + eps and its absolute-value form
        cond = aq / q                                                         # what a relative error of p becomes in 1 - p + eps
        lp, lq = np.log((p + eps).astype(T)), np.log(q)
        fp = -t / (p + eps) + (one - t) / q
        afp = t / (p + eps) + (one + t) / q * cond
        dot = (fp * p).sum(axis=1, keepdims=True, dtype=T)
        adot = (afp * p).sum(axis=1, keepdims=True, dtype=T)
        out.update(loss=(-(t * lp + (one - t) * lq)).sum(axis=1, dtype=T),
                   aloss=(t * (np.abs(lp) + one) + (one + t) * (np.abs(lq) + cond)).sum(axis=1, dtype=T),
                   g=p * (fp - dot), a=p * (afp + adot))
    elif fn == 'kld':
        lzs, lzt = np.log(zs).astype(T), np.log(zt).astype(T)
        logp, logt = (ls - ms) - lzs, (lt - mt) - lzt
        alogp = (als + als.max(axis=1, keepdims=True)) + np.abs(lzs)
        alogt = (alt + alt.max(axis=1, keepdims=True)) + np.abs(lzt)
        tsum = t.sum(axis=1, keepdims=True, dtype=T)
        pos = t > 0
        out.update(loss=np.where(pos, t * (logt - logp), T(0)).sum(axis=1, dtype=T),
                   aloss=np.where(pos, t * (alogt + alogp), T(0)).sum(axis=1, dtype=T), g=p * tsum - t, a=p * tsum + t)
    else:
        raise ValueError('Unknown consistency loss function {}'.format(fn))
    return out


def ce_pixel_terms(l, safe_label, dtype=np.float64, al=None):
    """loss = -log_softmax(l)[label], g = softmax - onehot, with their absolute-value forms; `safe_label` (N, H, W) in [0, C)"""
    T = dtype
    l = np.asarray(l, dtype=T)
    p, mx, z = _softmax(l, T)
    lz = np.log(z).astype(T)[:, 0]
    ll = np.take_along_axis(l, safe_label[:, None], axis=1)[:, 0]
    al = np.abs(l) if al is None else np.asarray(al, dtype=T)
    all_ = np.take_along_axis(al, safe_label[:, None], axis=1)[:, 0]
    hot = (np.arange(l.shape[1])[None, :, None, None] == safe_label[:, None]).astype(T)
    return dict(loss=-((ll - mx[:, 0]) - lz), aloss=(all_ + al.max(axis=1)) + np.abs(lz), g=p - hot, a=p + hot,
                L=al.max(axis=1))


def kappa(t32, t64, keys=('g', 'a')):
    """largest |fp32 - fp64| / (u32 * a * (1 + L)) over all elements (a = 0 elements must agree exactly)"""
    v, a = keys
    L = t64['L'] if t64[v].ndim == 3 else t64['L'][:, None]
    den = U32 * t64[a] * (1.0 + L)
    err = np.abs(t32[v].astype(np.float64) - t64[v])
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / den)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------ consistency
def consistency(l_stu, l_tea0, l_tea1, H, W, ac, mode='mix', fn='var', tau=0.97, per_pixel=False, ranges=None, mask=None,
                invert=True, um0=None, um1=None, ramp=1.0, weight=1.0, dtype=np.float64):
    """The unsupervised loss of the CutMix mean-teacher step on low-resolution logits (N, C, h, w).
    -> dict: scalars (consistency_loss, conf_rate [nan for tau <= 0], grad_scale, unsup_loss), grad (N, C, h, w) and, for the
    bounds: fg / fa (N, C, H, W) = f g_k and |f| a_k (1 + L), lm / alm (N, H, W) = the masked per-pixel values behind each of the two
    loss sums, d (h, w), conf (N, H, W), P, up_s / up_t (the upsampled logits)."""
    l_stu = np.asarray(l_stu, dtype=np.float64)
    N, C, h, w = l_stu.shape
    m = paste_bits(N, H, W, ranges, mask, invert)
    one = np.ones((N, H, W))
    u0 = one if um0 is None else np.asarray(um0, dtype=np.float64).reshape(N, H, W)
    u1 = one if um1 is None else np.asarray(um1, dtype=np.float64).reshape(N, H, W)
    if dtype is np.float64:
        up = lambda x: upsample(x, H, W, ac)
    else:
        up = lambda x: upsample_taps(x, H, W, ac, dtype)
    aup = lambda x: upsample(np.abs(np.asarray(x, dtype=np.float64)), H, W, ac)
    up_s, up_0, a_s, a_t = up(l_stu), up(l_tea0), aup(l_stu), aup(l_tea0)
    if mode == 'mix':
        up_t = np.where(m[:, None], up(l_tea1), up_0)
        a_t = np.where(m[:, None], aup(l_tea1), a_t)
        um = np.where(m, u1, u0)
    elif mode == 'cut':
        up_t = up_0
        um = np.where(m, u0, 0.0)
    else:
        raise ValueError('Unknown mask_mode {}'.format(mode))
    t = pixel_terms(up_s, up_t, fn, dtype, a_s, a_t)
    P = float(N * H * W)
    cf = (t['conf'].astype(np.float64) >= tau).astype(np.float64) if tau > 0 else one
    rate = cf.sum() / P if tau > 0 else float('nan')
    loss = t['loss'].astype(np.float64)
    if tau > 0 and per_pixel:
        pm, gs = um * cf, 1.0 / P
        closs = (loss * pm).sum() / P
    elif tau > 0:
        pm, gs = um, rate / P
        closs = rate * ((loss * um).sum() / P)
    else:
        pm, gs = um, 1.0 / P
        closs = (loss * um).sum() / P
    closs *= ramp
    gscale = gs * ramp * weight
    f = gscale * pm
    fg = f[:, None] * t['g'].astype(np.float64)
    fa = np.abs(f)[:, None] * t['a'].astype(np.float64) * (1.0 + t['L'].astype(np.float64))[:, None]
    _, _, d = matrices(h, w, H, W, ac)
    return dict(scalars=(closs, rate, gscale, closs * weight), grad=adjoint(fg, h, w, ac), fg=fg, fa=fa, d=d, conf=t['conf'],
                lm=loss * pm, alm=np.abs(pm) * t['aloss'].astype(np.float64) * (1.0 + t['L'].astype(np.float64)),
                value_scale=(rate if (tau > 0 and not per_pixel) else 1.0) * ramp / P, P=P, up_s=up_s, up_t=up_t, terms=t,
                h=h, w=w, ac=ac, fn=fn)


def grad_bound(r, kappa_fn=None):
    """(d + 2) u32 U^T|f g| + U^T(|f| K u32 a (1 + L)) for a result of `consistency` / `cross_entropy`"""
    K = MARGIN * KAPPA[kappa_fn or r['fn']]
    rel = (r['d'] + 2.0) * U32 * adjoint(np.abs(r['fg']), r['h'], r['w'], r['ac']) + K * U32 * adjoint(r['fa'], r['h'], r['w'], r['ac'])
    return rel + (r['d'] + 2.0) * TINY32 * (rel > 0)


def sum_depth(P):
    """longest fp32 addition chain of the loss sums: the pixels of one thread (two per thread in the tiled kernels, the trips of the
    grid-stride loop of 2048 x 256 threads in the direct ones), 6 shuffle steps of a wave, 4 waves; the partials meet in double"""
    return 2 + int(math.ceil(P / (2048.0 * 256.0))) + 6 + 4


def scalar_bound(r, kappa_fn=None):
    """bound of consistency_loss (times `weight` for unsup_loss; times 1 / value_scale for the raw sums): the per-pixel values at
    K u32 aloss (1 + L) each, their fp32 partial sums at depth sum_depth, and the final product / cast to fp32 (3 roundings)"""
    K = MARGIN * KAPPA_VALUE[kappa_fn or r['fn']]
    s = (sum_depth(r['P']) + 2.0) * U32 * np.abs(r['lm']).sum() + K * U32 * r['alm'].sum()
    return s * abs(r['value_scale']) + 3.0 * U32 * abs(r['scalars'][0])


# ------------------------------------------------------------------------------------------------------------ cross entropy
def cross_entropy(logits, labels, H, W, ac, ignore_index=255, weight=1.0, dtype=np.float64):
    """mean over the valid labels of -log_softmax(upsample(logits))[label]; a label equal to ignore_index, negative or >= C is
    skipped. -> dict: scalars (loss, grad_scale = weight / n_valid), n_valid, grad and the bound terms as in `consistency`."""
    logits = np.asarray(logits, dtype=np.float64)
    N, C, h, w = logits.shape
    y = np.asarray(labels).astype(np.int64).reshape(N, H, W)
    valid = (y != ignore_index) & (y >= 0) & (y < C)
    safe = np.where(valid, y, 0)
    up = upsample(logits, H, W, ac) if dtype is np.float64 else upsample_taps(logits, H, W, ac, dtype)
    t = ce_pixel_terms(up, safe, dtype, upsample(np.abs(logits), H, W, ac))
    nv = float(valid.sum())
    loss = t['loss'].astype(np.float64)
    vf = valid.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        val = np.float64((loss * vf).sum()) / nv
    gscale = weight / nv if nv > 0 else 0.0
    f = gscale * vf
    fg = f[:, None] * t['g'].astype(np.float64)
    fa = f[:, None] * t['a'].astype(np.float64) * (1.0 + t['L'].astype(np.float64))[:, None]
    _, _, d = matrices(h, w, H, W, ac)
    return dict(scalars=(val, gscale), n_valid=nv, grad=adjoint(fg, h, w, ac), fg=fg, fa=fa, d=d, lm=loss * vf,
                alm=vf * t['aloss'].astype(np.float64) * (1.0 + t['L'].astype(np.float64)), value_scale=(1.0 / nv if nv > 0 else 0.0),
                P=float(N * H * W), up=up, terms=t, valid=valid, h=h, w=w, ac=ac, fn='ce')


# ------------------------------------------------------------------------------------------------------------ tile arithmetic
TILE_W, TILE_H, FWD_TILE_H = 64, 4, 8
WT_COLS, WT_SPAN = 24, 20
LDS_OPT_IN, FWD_PATCH_LDS_MAX, LDS_MAX = 48 * 1024, 96 * 1024, 160 * 1024 - 4096
G_LD = TILE_W + 1


def _scale(in_size, out_size, ac):
    if ac:
        return np.float32(in_size - 1) / np.float32(out_size - 1) if out_size > 1 else np.float32(0)
    return np.float32(in_size) / np.float32(out_size)


def tile_max_cols(sx):
    return int(np.float32(TILE_W - 1) * sx) + 3


def tile_max_rows(sy, tile_h):
    return int(np.float32(tile_h - 1) * sy) + 3


def patch_floats(C, sy, sx, tile_h):
    return C * tile_max_rows(sy, tile_h) * tile_max_cols(sx)


def tile_lds_bytes(C, sy, sx, n_patches):
    return (TILE_H * C * G_LD + TILE_H * C * tile_max_cols(sx) + n_patches * patch_floats(C, sy, sx, TILE_H)) * 4


def tile_facts(C, h, w, H, W, ac, n_patches):
    """What the host side of csrc/loss_tiles.hpp decides for a geometry, from fp32 taps. n_patches = 3 (consistency) or 1 (CE)."""
    sy, sx = _scale(h, H, ac), _scale(w, W, ac)
    i0, i1, _, _ = R.bilinear_taps(w, W, ac, np.float32)
    y0, y1, _, _ = R.bilinear_taps(h, H, ac, np.float32)
    worst_cols = worst_span = worst_rows = 0
    tables = []
    for x0 in range(0, W, TILE_W):
        tw = min(TILE_W, W - x0)
        a, b = i0[x0:x0 + tw], i1[x0:x0 + tw]
        lo, n_cols = int(a[0]), int(b[-1] - a[0] + 1)
        span = 0
        for X in range(lo, lo + n_cols):
            touch = np.nonzero((a == X) | (b == X))[0]
            span = max(span, int(touch[-1] - touch[0] + 1))
        worst_cols, worst_span = max(worst_cols, n_cols), max(worst_span, span)
        tables.append(n_cols <= WT_COLS and span <= WT_SPAN)
    for yy in range(0, H, TILE_H):
        th = min(TILE_H, H - yy)
        worst_rows = max(worst_rows, int(y1[yy + th - 1] - y0[yy] + 1))
    ident = h == H and w == W
    lds = tile_lds_bytes(C, sy, sx, n_patches)
    fwd = n_patches * patch_floats(C, sy, sx, FWD_TILE_H) * 4
    assert worst_cols <= tile_max_cols(sx) and worst_rows <= tile_max_rows(sy, TILE_H), 'a tile outgrows its LDS rectangle'
    if ident:
        forward = backward = 'identity'
    else:
        forward = 'direct' if fwd > FWD_PATCH_LDS_MAX else ('tiled_optin' if fwd > LDS_OPT_IN else 'tiled')
        backward = 'error' if lds > LDS_MAX else ('tiled_optin' if lds > LDS_OPT_IN else 'tiled')
    return dict(r_n_cols=worst_cols, span=worst_span, r_n_rows=worst_rows, table_all=all(tables), table_any=any(tables),
                tiles_x=len(tables), lds=lds, fwd_lds=fwd, forward=forward, backward=backward,
                fused=(not ident) and lds <= LDS_MAX)


# ------------------------------------------------------------------------------------------------------------ shared cases
# the six (loss, mode, tau, per-pixel confidence) combinations of tests/test_gpu_parity.py
COMBOS = [('var', 'mix', 0.5, False), ('var', 'mix', 0.6, True), ('kld', 'cut', 0.5, True), ('bce', 'mix', 0.0, False),
          ('logits_var', 'cut', 0.0, False), ('logits_smoothl1', 'mix', 0.4, True)]
EVERYWHERE = [COMBOS[0], COMBOS[2]]           # `var` (its compile-time instantiation) and `kld` (the register-hungry one)

# name -> (N, C, h, w, H, W, align_corners, seed, all six combinations?, expected path facts [consistency, 3 patches])
#   loop = 'compare' (some tile leaves the wtab table) / 'table' (every tile on it)
GEOS = {
    'cmp33':    (2, 4, 17, 33, 33, 65, True, 1, False, dict(loop='compare', r_n_cols=33, backward='tiled', forward='tiled')),
    'tab2':     (2, 4, 8, 32, 32, 128, False, 1, False, dict(loop='table', tiles_x=2, backward='tiled', forward='tiled')),
    'tab2c19':  (2, 19, 8, 32, 32, 128, False, 5, False, dict(loop='table', tiles_x=2, backward='tiled', forward='tiled')),
    'tab2part': (2, 4, 8, 24, 32, 96, False, 1, True, dict(loop='table', tiles_x=2, backward='tiled', forward='tiled')),
    'span38':   (1, 21, 21, 21, 321, 321, False, 41, False, dict(loop='compare', span=38, backward='tiled', forward='tiled')),
    'span64':   (1, 21, 11, 11, 321, 321, True, 352, False, dict(loop='compare', r_n_cols=3, span=64, backward='tiled', forward='tiled')),
    'span42':   (2, 2, 3, 3, 50, 50, False, 1, False, dict(loop='compare', r_n_cols=3, span=42, backward='tiled', forward='tiled')),
    'one':      (2, 3, 1, 1, 9, 70, True, 1, False, dict(loop='compare', r_n_cols=1, span=64, tiles_x=2, backward='tiled', forward='tiled')),
    'onerow':   (2, 3, 1, 5, 5, 70, False, 1, False, dict(loop='compare', tiles_x=2, backward='tiled', forward='tiled')),
    'c1':       (2, 1, 3, 3, 50, 50, False, 1, False, dict(loop='compare', backward='tiled', forward='tiled')),
    'sy1':      (2, 5, 33, 70, 33, 140, True, 2, False, dict(loop='compare', r_n_cols=34, backward='tiled', forward='tiled')),
    'ratio2':   (1, 21, 160, 160, 321, 321, False, 53, False, dict(loop='compare', r_n_cols=34, backward='tiled_optin', forward='tiled_optin')),
    'ratio2s':  (2, 21, 32, 32, 65, 65, False, 4, True, dict(loop='compare', backward='tiled_optin', forward='tiled_optin')),
    'c40':      (1, 40, 41, 41, 321, 321, True, 214, False, dict(loop='table', backward='tiled_optin', forward='tiled')),
    'c60':      (1, 60, 41, 41, 321, 321, True, 52, False, dict(loop='table', backward='tiled_optin', forward='tiled')),
    'near1':    (1, 21, 60, 60, 65, 65, True, 6, True, dict(loop='compare', backward='tiled_optin', forward='direct')),
    'toobig':   (1, 32, 60, 60, 65, 65, True, 1, False, dict(loop='compare', backward='error', forward='direct', fused=False)),
    # the identity kernels (forward and backward, both losses) with a run-time class count; two tile columns' worth of pixels
    'identc3':  (2, 3, 9, 70, 9, 70, True, 1, False, dict(loop='compare', backward='identity', forward='identity', fused=False)),
    # ... and with a compile-time one (5): the instances the class-threshold kernels share with these are reached through it
    'identc5':  (2, 5, 9, 70, 9, 70, True, 1, False, dict(loop='compare', backward='identity', forward='identity', fused=False)),
    # the direct-gather forward of the CROSS ENTROPY (one rectangle: 46 x 9 x 62 floats = 100 KB > 96 KB), which only a run-time
    # class count reaches; its backward and fused launch are tiled (147 KB). No consistency backward at this size (three rectangles)
    'ce46':     (1, 46, 60, 60, 64, 64, True, 2, False, dict(loop='compare', backward='error', forward='direct', fused=False)),
}
# the dyadic geometries of the exact cases (C = 4, logits_var): every bilinear weight is a multiple of 2^-6
EXACT_GEOS = {
    'cmp33':    (2, 4, 17, 33, 33, 65, True),
    'tab2':     (2, 4, 8, 32, 32, 128, False),
    'tab2part': (2, 4, 8, 24, 32, 96, False),
}


def combos_of(name):
    return COMBOS if GEOS[name][8] else EVERYWHERE


def case_inputs(name, mode):
    """Gaussian logits (student x 2, teacher x 3), binary validity masks, two boxes per sample: fp32 arrays, the same for every route"""
    N, C, h, w, H, W, ac, seed = GEOS[name][:8]
    rng = np.random.RandomState(1000 * seed + C * H + w)
    ls = (rng.randn(N, C, h, w) * 2).astype(np.float32)
    l0 = (rng.randn(N, C, h, w) * 3).astype(np.float32)
    l1 = (rng.randn(N, C, h, w) * 3).astype(np.float32)
    um0 = (rng.rand(N, 1, H, W) > 0.2).astype(np.float32)
    um1 = (rng.rand(N, 1, H, W) > 0.2).astype(np.float32)
    ranges = boxes(rng, N, H, W, 2)
    return dict(ls=ls, l0=l0, l1=l1 if mode == 'mix' else None, um0=um0, um1=um1 if mode == 'mix' else None, ranges=ranges)


def boxes(rng, N, H, W, nb):
    """nb overlapping boxes per sample, each about half the map: int32 (N, nb, 4) = [y0, y1, x0, x1)"""
    out = np.zeros((N, nb, 4), dtype=np.int32)
    for n in range(N):
        for b in range(nb):
            bh, bw = max(1, (H * 2) // 3), max(1, (W * 2) // 3)
            y0, x0 = rng.randint(0, H - bh + 1), rng.randint(0, W - bw + 1)
            out[n, b] = (y0, y0 + bh, x0, x0 + bw)
    return out


def ce_inputs(name, label_dtype=np.uint8):
    N, C, h, w, H, W, ac, seed = GEOS[name][:8]
    rng = np.random.RandomState(2000 * seed + C * H + w)
    lo = (rng.randn(N, C, h, w) * 2).astype(np.float32)
    y = rng.randint(0, C, size=(N, H, W)).astype(np.int64)
    y[rng.rand(N, H, W) < 0.05] = 255
    return lo, y.astype(label_dtype)


def exact_inputs(name, mode):
    """integer logits in [-8, 8], binary um; mix: two overlapping boxes, cut: a float mask. cons_weight makes ramp * weight / P a
    power of two (ramp = 0.5)."""
    N, C, h, w, H, W, ac = EXACT_GEOS[name]
    rng = np.random.RandomState(77 + H + w)
    mk = lambda: rng.randint(-8, 9, size=(N, C, h, w)).astype(np.float32)
    ls, l0, l1 = mk(), mk(), mk()
    um0 = (rng.rand(N, 1, H, W) > 0.2).astype(np.float32)
    um1 = (rng.rand(N, 1, H, W) > 0.2).astype(np.float32)
    P = N * H * W
    ramp = 0.5
    weight = P / 2.0 ** math.ceil(math.log2(P)) / ramp * 0.5          # ramp * weight / P = 2^-(ceil(log2 P) + 1)
    d = dict(ls=ls, l0=l0, l1=l1 if mode == 'mix' else None, um0=um0, um1=um1 if mode == 'mix' else None, ramp=ramp, weight=weight)
    if mode == 'mix':
        d['ranges'] = boxes(rng, N, H, W, 2)
    else:
        d['mask'] = box_mask(boxes(rng, N, H, W, 2), H, W, True).astype(np.float32)[:, None] * 0.75 + 0.125      # 0.875 / 0.125
    return d


RAMP, WEIGHT = float(np.float32(0.9)), float(np.float32(0.7))          # what the C ABI receives: fp32 numbers
_cache = {}


def slim(r, tau=0.0):
    """what the tests keep of a reference result (the (N, C, H, W) arrays are dropped: the cache holds every case of the session)"""
    out = dict(scalars=r['scalars'], grad=r['grad'], bound=grad_bound(r), sbound=scalar_bound(r), P=r['P'])
    if 'conf' in r:
        out['conf_margin'] = float(np.abs(r['conf'] - tau).min()) if tau > 0 else float('inf')
    if 'n_valid' in r:
        out['n_valid'] = r['n_valid']
    return out


def reference(name, combo):
    """fp64 reference of one bounded consistency case (computed once per session)"""
    key = ('cons', name, combo)
    if key not in _cache:
        fn, mode, tau, pp = combo
        N, C, h, w, H, W, ac = GEOS[name][:7]
        i = case_inputs(name, mode)
        r = consistency(i['ls'], i['l0'], i['l1'], H, W, ac, mode, fn, tau, pp, ranges=i['ranges'], invert=True, um0=i['um0'],
                        um1=i['um1'], ramp=RAMP, weight=WEIGHT)
        _cache[key] = slim(r, tau)
    return _cache[key]


def ce_reference(name):
    key = ('ce', name)
    if key not in _cache:
        N, C, h, w, H, W, ac = GEOS[name][:7]
        lo, y = ce_inputs(name)
        _cache[key] = slim(cross_entropy(lo, y, H, W, ac, 255, 1.0))
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------ further cases
# name -> (geometry (N, C, h, w, H, W, ac), (loss, mode, tau, per_pixel), family of the bound, builder of the inputs)
def _gauss(geo, seed, scale=1.0, nb=2):
    N, C, h, w, H, W, ac = geo
    rng = np.random.RandomState(seed)
    d = dict(ls=(rng.randn(N, C, h, w) * 2 * scale).astype(np.float32), l0=(rng.randn(N, C, h, w) * 3 * scale).astype(np.float32),
             l1=(rng.randn(N, C, h, w) * 3 * scale).astype(np.float32), um0=(rng.rand(N, 1, H, W) > 0.2).astype(np.float32),
             um1=(rng.rand(N, 1, H, W) > 0.2).astype(np.float32))
    d['ranges'] = boxes(rng, N, H, W, nb)
    return d


def _uniform_teacher(geo, seed):
    d = _gauss(geo, seed)
    d['l0'] = np.full_like(d['l0'], 1.25)
    d['l1'] = np.full_like(d['l1'], -0.75)
    return d


def _with(d, **kw):
    d = dict(d)
    d.update(kw)
    return d


G_SY1, G_CMP, G_S42, G_TP = GEOS['sy1'][:7], GEOS['cmp33'][:7], GEOS['span42'][:7], GEOS['tab2part'][:7]
G_CMP3 = (3,) + G_CMP[1:]
EXTRA = {
    # exponentials underflow: t == 0 in KLD, 1 - p + eps == eps in BCE
    'pm60_kld':  (G_SY1, ('kld', 'cut', 0.5, True), lambda: _gauss(G_SY1, 40, 10.0)),
    'pm60_bce':  (G_SY1, ('bce', 'mix', 0.0, False), lambda: _gauss(G_SY1, 12, 10.0)),
    'pm60_bce4': (G_CMP, ('bce', 'mix', 0.0, False), lambda: _gauss(G_CMP, 13, 10.0)),
    # confidence exactly AT the threshold (1 / C for uniform logits): the pixels count and carry gradient
    'at_tau_c2': (G_S42, ('var', 'mix', 0.5, True), lambda: _uniform_teacher(G_S42, 14)),
    'at_tau_c4': (G_CMP, ('var', 'mix', 0.25, True), lambda: _uniform_teacher(G_CMP, 15)),
    # validity weights
    'um_zero':   (G_TP, ('var', 'mix', 0.0, False), lambda: _with(_gauss(G_TP, 16), um0=np.zeros((G_TP[0], 1, G_TP[4], G_TP[5]), np.float32),
                                                                 um1=np.zeros((G_TP[0], 1, G_TP[4], G_TP[5]), np.float32))),
    'um_0.3':    (G_TP, ('var', 'mix', 0.0, False), lambda: _with(_gauss(G_TP, 17), um0=np.full((G_TP[0], 1, G_TP[4], G_TP[5]), 0.3, np.float32))),
    # three samples on a comparing-loop geometry: accumulation into a non-zero grad_out, samples=(1, 3)
    'three':     (G_CMP3, ('kld', 'mix', 0.0, False), lambda: _gauss(G_CMP3, 18)),
}
for _nb in (0, 1, 3):
    EXTRA['boxes%d' % _nb] = (G_TP, ('var', 'mix', 0.5, False), (lambda nb: (lambda: _gauss(G_TP, 20 + nb, nb=nb)))(_nb))
AT_TAU = ('at_tau_c2', 'at_tau_c4')


def extra_reference(name, invert=True, full=False):
    key = ('extra', name, invert)
    if key not in _cache or full:
        geo, (fn, mode, tau, pp), build = EXTRA[name]
        N, C, h, w, H, W, ac = geo
        i = build()
        r = consistency(i['ls'], i['l0'], i['l1'] if mode == 'mix' else None, H, W, ac, mode, fn, tau, pp, ranges=i['ranges'], invert=invert,
                        um0=i['um0'], um1=i['um1'] if mode == 'mix' else None, ramp=RAMP, weight=WEIGHT)
        if full:
            return r
        _cache[key] = slim(r, tau)
    return _cache[key]


def ce_i64_inputs():
    """int64 labels with negatives, values >= C, the ignore value and values beyond 2^31"""
    N, C, h, w, H, W, ac = G_TP
    rng = np.random.RandomState(31)
    lo = (rng.randn(N, C, h, w) * 2).astype(np.float32)
    y = rng.randint(-2, C + 3, size=(N, H, W)).astype(np.int64)
    y[rng.rand(N, H, W) < 0.05] = 255
    y[0, 0, :4] = (-(2 ** 40), 2 ** 33 + 1, 2 ** 31, -1)
    return lo, y
