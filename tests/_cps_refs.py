"""Test helper: the fp64 restatement, in plain numpy, of the cross-pseudo-supervision labels (csrc/cps.hip) -- bilinear upsample in
fp64 (the restatement tests/_tta_refs.py holds against torch), the select by the mix mask, argmax, the largest softmax probability,
validity, threshold, the four counts --, the margins its cases must keep, the cases the CPU and GPU tests share, and the restatement
of one whole CPS iteration on the CPU oracle. Nothing here imports the product."""
import functools
import struct

import numpy as np
import torch

import _hostcheck
import _tta_refs as T

GAP = 1e-4          # the two largest upsampled logits of a pixel differ by at least this (the project's margin for this arithmetic)
CONF = 1e-5         # |conf - tau| is at least this when tau > 0
TAU = 0.6
IGNORE = 255


def box_mask(ranges, size, invert):
    """(n, nb, 4) half-open [y0, y1, x0, x1] -> bool (n, H, W): the parity of the boxes over a pixel under `invert` (pixel_math.hpp's
    box_mask_bit), True = take image 1"""
    ranges = np.asarray(ranges)
    H, W = size
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    out = np.zeros((ranges.shape[0], H, W), dtype=bool)
    for i, boxes in enumerate(ranges):
        for y0, y1, x0, x1 in boxes:
            out[i] ^= (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
    return out if invert else ~out


def _net(l0, l1, m, size, align):
    u = np.where(m[:, None], T.upsample(l1, size, align), T.upsample(l0, size, align))
    pred = u.argmax(axis=1)                                           # first index on a tie, the first NaN if there is one
    c = u.shape[1]
    if c > 1:
        top = np.sort(u, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(pred.shape, np.inf)
    with np.errstate(invalid='ignore'):
        conf = T.softmax(u, 1).max(axis=1) if not np.isnan(u).any() else np.take_along_axis(T.softmax(u, 1), pred[:, None], 1)[:, 0]
    return pred, conf, gap


def cps_labels(l0_a, l1_a, l0_b, l1_b, size, align, m, um0=None, um1=None, tau=0.0):
    """logits (n,c,h,w), m bool (n,H,W) "take image 1", um0 / um1 optional (n,H,W) -> dict(label_a, label_b uint8 (n,H,W), stats
    int64[4] = n_valid, kept_a, kept_b, agree; gap: the smallest top-two gap over both networks and all pixels; conf_margin: the
    smallest |conf - tau| over both networks and all pixels (inf for tau <= 0))"""
    m = np.asarray(m, dtype=bool)
    one = np.ones(m.shape, dtype=bool)
    valid = np.where(m, one if um1 is None else np.asarray(um1) >= 0.5, one if um0 is None else np.asarray(um0) >= 0.5)
    out, kept, gaps, margins, preds = [], [], [], [], []
    for l0, l1 in ((l0_a, l1_a), (l0_b, l1_b)):
        pred, conf, gap = _net(l0, l1, m, size, align)
        with np.errstate(invalid='ignore'):
            keep = valid & ((conf >= np.float64(np.float32(tau))) if tau > 0 else one)
        out.append(np.where(keep, pred, IGNORE).astype(np.uint8))
        kept.append(int(keep.sum()))
        gaps.append(float(gap.min()))
        margins.append(float(np.abs(conf - np.float64(np.float32(tau))).min()) if tau > 0 else float('inf'))
        preds.append(pred)
    stats = np.array([int(valid.sum()), kept[0], kept[1], int((valid & (preds[0] == preds[1])).sum())], dtype=np.int64)
    return dict(label_a=out[0], label_b=out[1], stats=stats, gap=min(gaps), conf_margin=min(margins), pred_a=preds[0], pred_b=preds[1])


# ------------------------------------------------------------------------------------------------------------------ shared cases
# name -> (n, c, (h, w), (H, W)): the smallest shapes at which the walk can go wrong
#   main      H * W = 2050 is no multiple of four: sample starts are unaligned, head and tail labels are written byte by byte
#   c21       an odd pixel count; the 21-class instantiation
#   ident     the logits have the output's size: no interpolation
#   one       input size 1
#   c64       the class limit
#   tab2c19   3072 pixels per sample: three workgroups per sample; the 19-class instantiation
GEOMETRIES = {
    'main': (3, 5, (6, 7), (41, 50)),
    'c21': (2, 21, (5, 5), (33, 33)),
    'ident': (2, 2, (9, 70), (9, 70)),
    'one': (1, 3, (1, 1), (9, 70)),
    'c64': (1, 64, (3, 4), (17, 19)),
    'tab2c19': (2, 19, (8, 24), (32, 96)),
}

# (geometry, align_corners, mask kind) -> seed: the first seed from 11 upwards at which the fp64 reference keeps both margins at EVERY
# pixel with tau = TAU (tests/test_cps_cpu.py::test_case_margins re-checks them; no pixel is ever left out of a comparison).
#   'rand'   mask = rand > 0.5, given as a float mask
#   'box'    two boxes per sample, given as a range table under invert=True and as the float mask that equals it
#   'xbox'   the same under invert=False
KINDS = ('rand', 'box', 'xbox')


def draw(name, align, kind, seed):
    """the recipe: one generator; the four logit tensors in the order l0_a, l1_a, l0_b, l1_b, then the mask, then (for the box kinds)
    the box corners; the validity maps come from a generator of their own"""
    n, c, (h, w), (H, W) = GEOMETRIES[name]
    g = torch.Generator().manual_seed(seed)
    lg = [(torch.randn(n, c, h, w, generator=g) * 3).numpy() for _ in range(4)]
    mask = (torch.rand(n, 1, H, W, generator=g) > 0.5).numpy()[:, 0]
    ranges, invert = None, True
    if kind != 'rand':
        ys = torch.randint(0, H + 1, (n, 2, 2), generator=g).numpy()
        xs = torch.randint(0, W + 1, (n, 2, 2), generator=g).numpy()
        ranges = np.stack([ys.min(-1), ys.max(-1), xs.min(-1), xs.max(-1)], axis=-1).astype(np.int32)
        invert = kind == 'box'
        mask = box_mask(ranges, (H, W), invert)
    g2 = torch.Generator().manual_seed(seed + 1000)
    um0 = (torch.rand(n, H, W, generator=g2) > 0.2).float().numpy()
    um1 = (torch.rand(n, H, W, generator=g2) > 0.2).float().numpy()
    return dict(logits=lg, m=mask, mask=mask.astype(np.float32), ranges=ranges, invert=invert, um0=um0, um1=um1, size=(H, W),
                align=align)


def margins_hold(inp):
    ref = cps_labels(*inp['logits'], inp['size'], inp['align'], inp['m'], tau=TAU)
    return ref['gap'] >= GAP and ref['conf_margin'] >= CONF


def search(name, align, kind, first=11):
    seed = first
    while not margins_hold(draw(name, align, kind, seed)):
        seed += 1
    return seed


SEEDS = {
    ('main', True, 'rand'): 15,
    ('main', True, 'box'): 12,
    ('main', True, 'xbox'): 13,
    ('main', False, 'rand'): 14,
    ('main', False, 'box'): 13,
    ('main', False, 'xbox'): 15,
    ('c21', True, 'rand'): 11,
    ('c21', True, 'box'): 12,
    ('c21', True, 'xbox'): 11,
    ('c21', False, 'rand'): 11,
    ('c21', False, 'box'): 11,
    ('c21', False, 'xbox'): 15,
    ('ident', True, 'rand'): 11,
    ('ident', True, 'box'): 11,
    ('ident', True, 'xbox'): 11,
    ('ident', False, 'rand'): 11,
    ('ident', False, 'box'): 11,
    ('ident', False, 'xbox'): 11,
    ('one', True, 'rand'): 11,
    ('one', True, 'box'): 11,
    ('one', True, 'xbox'): 11,
    ('one', False, 'rand'): 11,
    ('one', False, 'box'): 11,
    ('one', False, 'xbox'): 11,
    ('c64', True, 'rand'): 12,
    ('c64', True, 'box'): 11,
    ('c64', True, 'xbox'): 13,
    ('c64', False, 'rand'): 11,
    ('c64', False, 'box'): 11,
    ('c64', False, 'xbox'): 11,
    ('tab2c19', True, 'rand'): 13,
    ('tab2c19', True, 'box'): 20,
    ('tab2c19', True, 'xbox'): 13,
    ('tab2c19', False, 'rand'): 12,
    ('tab2c19', False, 'box'): 11,
    ('tab2c19', False, 'xbox'): 12,
}


@functools.lru_cache(maxsize=None)
def case(name, align, kind):
    """-> the inputs of a case, drawn once and left unchanged"""
    return draw(name, align, kind, SEEDS[(name, align, kind)])


@functools.lru_cache(maxsize=None)
def reference(name, align, kind, with_um, tau):
    """-> the fp64 reference of a case's variant, computed once and left unchanged"""
    inp = case(name, align, kind)
    return cps_labels(*inp['logits'], inp['size'], inp['align'], inp['m'], inp['um0'] if with_um else None,
                      inp['um1'] if with_um else None, tau)


def variants():
    """every (kind, with_um, tau) a geometry runs with"""
    return [(kind, um, tau) for kind in KINDS for um in (False, True) for tau in (0.0, TAU)]


# ------------------------------------------------------------------------------------------------------------------ host driver
def hostcheck_run(exe, logits, size, align, mask=None, ranges=None, invert=True, um0=None, um1=None, tau=0.0, vec=True,
                  expect_code=0, **over):
    """one request through the host driver -> dict(label_a, label_b, stats), or None when it ends with `expect_code` != 0.
    `over`: header fields sent as they are, whatever the arrays' shapes say."""
    n, c, h, w = logits[0].shape
    head = dict(n=n, c=c, h=h, w=w, H=size[0], W=size[1], n_boxes=0 if ranges is None else int(np.asarray(ranges).shape[1]))
    head.update(over)
    header = struct.pack('<12if', head['n'], head['c'], head['h'], head['w'], head['H'], head['W'], int(align), head['n_boxes'],
                         int(invert), int(um0 is not None), int(um1 is not None), int(vec), float(tau))
    blocks = [(t, np.float32) for t in logits]
    blocks.append((ranges, np.int32) if ranges is not None else (mask, np.float32))
    blocks += [(t, np.float32) for t in (um0, um1) if t is not None]
    raw = _hostcheck.run(exe, header, blocks, expect_code)
    if raw is None:
        return None
    shape = (n,) + tuple(size)
    return _hostcheck.split(raw, [('label_a', np.uint8, shape), ('label_b', np.uint8, shape), ('stats', np.int64, (4,))])


def same(got, ref):
    """labels and all four counts, every pixel"""
    assert np.array_equal(got['label_a'], ref['label_a'])
    assert np.array_equal(got['label_b'], ref['label_b'])
    assert np.array_equal(np.asarray(got['stats']), ref['stats']), (got['stats'], ref['stats'])


def mask_args(inp, as_ranges):
    """how a case's mask is handed over: its box table under its `invert`, or the float mask"""
    if as_ranges:
        return dict(ranges=inp['ranges'], invert=inp['invert'])
    return dict(mask=inp['mask'])


# ------------------------------------------------------------------------------------------------------------------ the iteration
def net_state(spec, seed):
    """random, non-degenerate weights and BatchNorm statistics for oracle.deeplab2's `state_spec` (the recipe of tests/test_gpu_ict.py);
    two seeds give the two differently initialised networks"""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for k, (shape, dt) in spec.items():
        if dt == torch.int64:
            st[k] = torch.zeros(shape, dtype=torch.int64)
        elif len(shape) == 4:
            st[k] = torch.randn(shape, generator=g) * (1.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith('running_var'):
            st[k] = 0.8 + 0.4 * torch.rand(shape, generator=g)
        elif k.endswith('running_mean'):
            st[k] = 0.1 * torch.randn(shape, generator=g)
        elif k.endswith('.weight'):
            st[k] = 0.6 + 0.8 * torch.rand(shape, generator=g)
        else:
            st[k] = 0.1 * torch.randn(shape, generator=g)
    return st


def step_data(seed, n, c, H, W):
    """the supervised batch, two unsupervised images, their validity maps and a box table with one box per sample"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, H, W, generator=g)
    y = torch.randint(0, c, (n, 1, H, W), generator=g)
    y[torch.rand(n, 1, H, W, generator=g) < 0.05] = 255
    ux0, ux1 = torch.randn(n, 3, H, W, generator=g), torch.randn(n, 3, H, W, generator=g)
    um0 = (torch.rand(n, 1, H, W, generator=g) > 0.2).float()
    um1 = (torch.rand(n, 1, H, W, generator=g) > 0.2).float()
    y0 = torch.randint(0, H // 2, (n,), generator=g)
    x0 = torch.randint(0, W // 2, (n,), generator=g)
    ranges = torch.stack([y0, y0 + H // 2, x0, x0 + W // 2], dim=1).reshape(n, 1, 4).to(torch.int32)
    return dict(x=x, y=y, ux0=ux0, ux1=ux1, um0=um0, um1=um1, ranges=ranges)


def cps_iteration(lowres_a, lowres_b, data, tau=0.0, ramp=1.0, invert=True):
    """One CPS iteration restated on the CPU. `lowres_k(x)` -> network k's low-resolution logits (oracle.deeplab2.forward_lowres under
    frozen BatchNorm); aligned corners. -> dict(sup_loss, consistency_loss, conf_rate, agreement, labels: the cps_labels reference
    (with its top-two gap), lows: the six low-resolution logit tensors L0_a, L1_a, L0_b, L1_b, S_a, S_b)"""
    import torch.nn.functional as F
    x, y, ux0, ux1 = data['x'], data['y'], data['ux0'], data['ux1']
    size = tuple(x.shape[2:4])
    m = box_mask(data['ranges'].numpy(), size, invert)

    def ce(lo, labels):
        logp = F.log_softmax(F.interpolate(lo.double(), size=size, mode='bilinear', align_corners=True), dim=1)
        valid = labels != IGNORE
        picked = torch.gather(logp, 1, torch.where(valid, labels, torch.zeros_like(labels))[:, None])[:, 0]
        return float(-(picked * valid).sum() / valid.sum()) if bool(valid.any()) else 0.0

    with torch.no_grad():
        lows = [lowres_a(ux0), lowres_a(ux1), lowres_b(ux0), lowres_b(ux1)]
        ref = cps_labels(*[t.numpy() for t in lows], size, True, m, data['um0'][:, 0].numpy(), data['um1'][:, 0].numpy(), tau)
        mt = torch.from_numpy(m[:, None].astype(np.float32))
        x_mix = ux0 * (1 - mt) + ux1 * mt
        lows += [lowres_a(x_mix), lowres_b(x_mix)]
        loss_a = ce(lows[4], torch.from_numpy(ref['label_b'].astype(np.int64)))
        loss_b = ce(lows[5], torch.from_numpy(ref['label_a'].astype(np.int64)))
        sup = 0.5 * (ce(lowres_a(x), y[:, 0].long()) + ce(lowres_b(x), y[:, 0].long()))
    st = ref['stats']
    return dict(sup_loss=sup, consistency_loss=(loss_a + loss_b) * ramp, conf_rate=float(st[1] + st[2]) / (2.0 * m.size),
                agreement=float(st[3]) / float(st[0]), labels=ref, lows=lows, m=m)
