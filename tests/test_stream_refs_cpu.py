"""
CPU: the references of tests/_stream_refs.py against torch in fp64 (F.interpolate and autograd, torch.cat / expand,
F.max_pool2d(return_indices=True), F.conv2d with one-hot weights), at every geometry tests/test_gpu_stream_kernels.py uses --
agreement <= 1e-12 relative -- and the input-quality conditions those GPU tests rely on (the share of undecided argmax pixels).
This is what makes the references trustworthy without a GPU.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stream_refs as R

REL = 1e-12


def _close(a, b, what=''):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()), 1e-300) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    assert err <= REL * scale, (what, err, scale)


ALL_GEOS = R.BILINEAR_GEOS + [R.NHWC_WRAP_GEO, R.NCHW_WRAP_FWD, R.NCHW_WRAP_BWD]
_ids = lambda g: '{}x{}to{}x{}'.format(g[0][0], g[0][1], g[1][0], g[1][1])


@pytest.mark.parametrize('align', [False, True], ids=['half_pixel', 'align_corners'])
@pytest.mark.parametrize('geo', ALL_GEOS, ids=_ids)
def test_bilinear_and_adjoint_vs_interpolate_fp64(geo, align):
    (h, w), (H, W) = geo
    g = torch.Generator().manual_seed(h * 1000 + W)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    up = F.interpolate(x, size=(H, W), mode='bilinear', align_corners=align)
    up.backward(dy)
    for layout, perm, back in (('nchw', (0, 1, 2, 3), (0, 1, 2, 3)), ('nhwc', (0, 2, 3, 1), (0, 3, 1, 2))):
        xn = np.ascontiguousarray(x.detach().numpy().transpose(perm))
        gn = np.ascontiguousarray(dy.numpy().transpose(perm))
        ref, A = R.upsample_bilinear(xn, (H, W), align, layout)
        _close(ref.transpose(back), up.detach().numpy(), 'forward ' + layout)
        upa = F.interpolate(x.detach().abs(), size=(H, W), mode='bilinear', align_corners=align)
        _close(A.transpose(back), upa.numpy(), 'A ' + layout)
        adj, Aa, d = R.upsample_bilinear_adjoint(gn, (h, w), align, layout)
        _close(adj.transpose(back), x.grad.numpy(), 'adjoint ' + layout)
        assert (Aa >= np.abs(adj) * (1 - 1e-12)).all() and ((d > 0) | (Aa == 0)).all()      # untouched sources: d = 0, A = 0
        # <U x, y> = <x, U^T y>
        lhs, rhs = R.dot64(ref, gn), R.dot64(xn, adj)
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(ref * gn).sum())


@pytest.mark.parametrize('align', [False, True], ids=['half_pixel', 'align_corners'])
@pytest.mark.parametrize('geo', ALL_GEOS, ids=_ids)
def test_fp32_weights_are_torchs_fp32_weights(geo, align):
    """weight_dtype=np.float32 restates the arithmetic F.interpolate does on an fp32 tensor: interpolating the unit vectors along one
    axis returns torch's weights themselves (1 * w + 0 is exact), bit for bit."""
    for n_in, n_out in zip(geo[0], geo[1]):
        M, _ = R.bilinear_matrix(n_in, n_out, align, np.float32)
        eye = torch.eye(n_in, dtype=torch.float32).view(1, n_in, n_in, 1)           # channel j = unit vector j along H
        got = F.interpolate(eye, size=(n_out, 1), mode='bilinear', align_corners=align)[0, :, :, 0].numpy().T   # (out, in)
        assert np.array_equal(M.astype(np.float32), got)
        if n_in > 1:            # (one source element: both taps are that element and torch's sum of the two weights is rounded)
            assert np.array_equal(M, got.astype(np.float64))
        M64, _ = R.bilinear_matrix(n_in, n_out, align, np.float64)
        assert np.abs(M - M64).max() <= 4 * R.U32 * max(n_in, 1)                    # and close to the fp64 definition


def test_concat_broadcast_and_adjoint_vs_cat_expand():
    g = torch.Generator().manual_seed(3)
    N, H, W = 2, 6, 5
    xs = [torch.randn(N, H, W, 8, generator=g, dtype=torch.float64, requires_grad=True),
          torch.randn(N, 1, 1, 16, generator=g, dtype=torch.float64, requires_grad=True),
          torch.randn(N, H, W, 24, generator=g, dtype=torch.float64, requires_grad=True)]
    dy = torch.randn(N, H, W, 48, generator=g, dtype=torch.float64)
    ref = torch.cat([xs[0], xs[1].expand(N, H, W, 16), xs[2]], dim=3)
    ref.backward(dy)
    got = R.concat_broadcast([x.detach().numpy() for x in xs])
    assert np.array_equal(got, ref.detach().numpy())
    for (r, A), x in zip(R.concat_broadcast_adjoint(dy.numpy(), [tuple(x.shape) for x in xs]), xs):
        _close(r, x.grad.numpy(), 'concat adjoint')
        assert (A >= np.abs(r) * (1 - 1e-12)).all()
    # every input 1 x 1: a plain concat
    ys = [np.ones((2, 1, 1, 8)), np.zeros((2, 1, 1, 16))]
    assert R.concat_broadcast(ys).shape == (2, 1, 1, 24)
    assert R.concat_broadcast_adjoint(np.ones((2, 1, 1, 24)), [y.shape for y in ys])[1][0].shape == (2, 1, 1, 16)


@pytest.mark.parametrize('rows', [(1, 1), (3, 11), (33, 33)])
def test_mean_and_sum_vs_torch(rows):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, rows[0], rows[1], 8, generator=g, dtype=torch.float64)
    ref, A = R.mean_over_pixels(x.numpy())
    _close(ref, x.mean(dim=(1, 2), keepdim=True).numpy())
    _close(A, x.abs().mean(dim=(1, 2), keepdim=True).numpy())
    xs = [torch.randn(5, 8, generator=g, dtype=torch.float64) for _ in range(6)]
    for k in range(1, 7):
        s, As = R.sum_k([t.numpy() for t in xs[:k]])
        _close(s, torch.stack(xs[:k]).sum(0).numpy())
        _close(As, torch.stack(xs[:k]).abs().sum(0).numpy())
    assert R.rows_reduce_depth(1) == 33 and R.rows_reduce_depth(33) == 34 and R.rows_reduce_depth(16641) == 553


def _aspp_tap_lists():
    taps18 = [(ky * d - d, kx * d - d) for d in (6, 12) for ky in range(3) for kx in range(3)]
    return [taps18, [(0, 0)], [(-3, 2)]]


_ASPP_CPU = [(m, c) for m in R.ASPP_MAPS[:3] + [(2, 13, 29)] for c in R.ASPP_CLASSES] + [(R.ASPP_MAPS[3], 2), ((7, 65, 129), 2), ((8, 65, 129), 2)]


@pytest.mark.parametrize('nhw,C', _ASPP_CPU, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_aspp_gather_and_spread_vs_one_hot_convolutions(nhw, C):
    """the shift-gather is a convolution whose weight for (class c, tap k) is one-hot on input channel k*C + c at offset (dy, dx);
    the spread is its adjoint (autograd), transposed to NHWC"""
    N, H, W = nhw
    g = torch.Generator().manual_seed(C * 100 + H)
    for taps in _aspp_tap_lists():
        T = len(taps)
        zc = (T * C + 7) // 8 * 8
        z = torch.randn(N, zc, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        bias = torch.randn(C, generator=g, dtype=torch.float64)
        dl = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
        out = bias.view(1, C, 1, 1).expand(N, C, H, W).clone()
        for k, (dy, dx) in enumerate(taps):
            r = max(abs(dy), abs(dx))
            wgt = torch.zeros(C, 1, 2 * r + 1, 2 * r + 1, dtype=torch.float64)         # class c <- channel k*C + c at (dy, dx)
            wgt[:, 0, r + dy, r + dx] = 1.0
            out = out + F.conv2d(z[:, k * C:(k + 1) * C], wgt, None, 1, r, groups=C)
        out.backward(dl)
        ref, A = R.aspp_gather(z.detach().numpy(), bias.numpy(), taps, C)
        _close(ref, out.detach().numpy(), 'gather')
        assert (A >= np.abs(ref) * (1 - 1e-12)).all()
        ref0, _ = R.aspp_gather(z.detach().numpy(), None, taps, C)
        _close(ref0 + bias.numpy().reshape(1, C, 1, 1), ref, 'bias=None')
        D = R.aspp_spread(dl.numpy(), taps, zc)
        assert np.array_equal(D, z.grad.numpy().transpose(0, 2, 3, 1))               # data movement: exact
        assert not D[..., T * C:].any()


@pytest.mark.parametrize('ceil_mode', [False, True], ids=['floor', 'ceil'])
@pytest.mark.parametrize('shape', R.POOL_SHAPES[:5] + [(1, 20, 33, 8)], ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_and_routed_backward_vs_torch(shape, ceil_mode):
    s = R.pool_input(shape, seed=shape[1] * 31 + shape[2])
    st = torch.from_numpy(s).double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    relu = F.relu(st)
    p, ind = F.max_pool2d(relu, 3, 2, 1, ceil_mode=ceil_mode, return_indices=True)
    n, hs, ws, c = shape
    assert (R.pool_out_size(hs, ceil_mode), R.pool_out_size(ws, ceil_mode)) == tuple(p.shape[2:])
    got = R.maxpool3x3s2(np.maximum(s, 0), ceil_mode)
    assert np.array_equal(got, p.detach().permute(0, 2, 3, 1).numpy().astype(np.float32))
    # torch's flat argmax -> ky * 3 + kx of its window
    hp, wp = p.shape[2:]
    iy, ix = (ind // ws).numpy(), (ind % ws).numpy()
    py, px = np.arange(hp).reshape(1, 1, hp, 1), np.arange(wp).reshape(1, 1, 1, wp)
    idx = ((iy - (2 * py - 1)) * 3 + (ix - (2 * px - 1))).transpose(0, 2, 3, 1)
    assert idx.min() >= 0 and idx.max() <= 8
    val, inside = R.maxpool_window_value(np.maximum(s, 0), idx, ceil_mode)
    assert inside.all() and np.array_equal(val, got)
    rng = np.random.RandomState(5)
    dp = rng.randint(-8, 9, size=got.shape).astype(np.float64)
    p.backward(torch.from_numpy(dp).permute(0, 3, 1, 2))
    ds = R.maxpool3x3s2_relu_backward(dp, idx, s)
    assert np.array_equal(ds, st.grad.permute(0, 2, 3, 1).numpy())       # relu's gate = [s > 0]; integers: exact


def test_pool_inputs_have_ties_and_zeros():
    """the GPU pool tests want windows with several equal maxima (the routing must not depend on the tie rule) and exact zeros"""
    for shape in R.POOL_SHAPES[2:5]:
        s = R.pool_input(shape, seed=shape[1] * 31 + shape[2])
        assert (s == 0).mean() > 0.02
        p = R.maxpool3x3s2(s, True)
        P = R._pool_padded(s, p.shape[1], p.shape[2], -np.inf)
        hp, wp = p.shape[1:3]
        hits = sum((P[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :] == p).astype(int) for ky in range(3) for kx in range(3))
        assert (hits > 1).mean() > 0.05


def test_confusion_vs_loops():
    rng = np.random.RandomState(6)
    C = 5
    t = rng.randint(-3, 9, size=500)
    t[::7] = 255
    p = rng.randint(0, 7, size=500)
    for ign in (None, 255, 3):
        want = np.zeros((C, C), dtype=np.int64)
        for a, b in zip(t, p):
            if 0 <= a < C and b < C and a != ign:
                want[a, b] += 1
        assert np.array_equal(R.confusion(t, p, C, ign), want)
    up = rng.randn(2, 4, 3, 3)
    up[0, 1, 0, 0] = up[0, 3, 0, 0] = 9.0                     # tie: the first index
    top, margin = R.argmax_margin(up)
    assert top[0, 0, 0] == 1 and margin[0, 0, 0] == 0.0
    assert np.array_equal(top, torch.from_numpy(up).argmax(1).numpy())


@pytest.mark.parametrize('case', R.EVAL_CASES, ids=lambda c: 'x'.join(map(str, c[:7])))
def test_undecided_argmax_pixels_are_rare(case):
    """The GPU test compares the kernel's class with the reference's wherever top1 - top2 > 2 * eps, eps = 4 * u32 * max |logit|.
    That says something only if nearly every pixel is decided: <= 1e-4 of all for the seeds and the scale used there."""
    n, c, h, w, H, W, align, _ = case
    lo = R.eval_logits(case)
    up, _ = R.upsample_bilinear(lo, (H, W), align, 'nchw', np.float32)
    if (h, w) == (H, W):
        assert np.array_equal(up, lo.astype(np.float64))
    eps = 4 * R.U32 * float(np.abs(lo).max())
    _, margin = R.argmax_margin(up)
    share = float((margin <= 2 * eps).mean())
    print('undecided share', share)
    assert share <= 1e-4
