"""
GPU: hole filling of binary predictions on the device (csrc/fillholes.hip, ops.fill_holes, EvaluatorIoU with fill_holes).

The reference everywhere is scipy.ndimage.binary_fill_holes(p != 0) per image, computed on the host inside the test. The result
is unique (a background pixel survives iff it is 4-connected through background to the outside of the image), so every
comparison is torch.equal / array_equal: no tolerances. The kernel labels 64 x 64 tiles (kernel constant kFillTile) and merges
them along the seams, so the shapes sit on and around multiples of 64, span several tiles, and end in partial tiles.
"""
import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE = 64


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


def _ref(p):
    """(H,W) or (N,H,W) integer map -> uint8 {0,1}, each image filled on its own"""
    p = np.asarray(p)
    if p.ndim == 2:
        return ndimage.binary_fill_holes(p != 0).astype(np.uint8)
    return np.stack([_ref(q) for q in p])


def _fill(ops, p, **kw):
    out, cm = ops.fill_holes(torch.from_numpy(np.ascontiguousarray(p, dtype=np.uint8)).to(DEV), **kw)
    return out, cm


def _check(ops, p):
    want = torch.from_numpy(_ref(p))
    out, cm = _fill(ops, p)
    assert cm is None and out.dtype == torch.uint8 and tuple(out.shape) == tuple(np.shape(p))
    assert torch.equal(out.cpu(), want)
    return want.numpy()


def _ring3():
    p = np.ones((3, 3), np.uint8)
    p[1, 1] = 0
    return p


DEGENERATE = {
    '1x1_background': np.zeros((1, 1), np.uint8),
    '1x1_foreground': np.ones((1, 1), np.uint8),
    '1x7_mixed': np.array([[0, 1, 0, 0, 1, 1, 0]], np.uint8),
    '7x1_mixed': np.array([[1, 0, 1, 1, 0, 0, 1]], np.uint8).T.copy(),
    '2x2_background': np.zeros((2, 2), np.uint8),
    '3x3_ring': _ring3(),
}


@pytest.mark.parametrize('name', sorted(DEGENERATE))
def test_degenerate_shapes(ops, name):
    got = _check(ops, DEGENERATE[name])
    if name == '3x3_ring':
        assert got[1, 1] == 1


def test_diagonal_contact_does_not_connect(ops):
    p = np.ones((5, 5), np.uint8)
    p[0, 0] = p[1, 1] = 0
    got = _check(ops, p)
    assert got[1, 1] == 1 and got[0, 0] == 0


# H and W from {31, 32, 33, 63, 64, 65, 129}: one below / on / one above the tile edge (64 is the kernel's own), half a tile, two
# tiles plus one pixel
TILE_EDGE_SHAPES = [(31, 129), (32, 64), (33, 65), (63, 63), (63, 64), (64, 63), (64, 64), (64, 65), (65, 64), (65, 65), (129, 31),
                    (129, 129), (65, 33), (32, 129)]


@pytest.mark.parametrize('shape', TILE_EDGE_SHAPES, ids=lambda s: '{}x{}'.format(*s))
def test_tile_edges(ops, shape):
    H, W = shape
    rng = np.random.default_rng(7 * H + W)
    _check(ops, (rng.random((H, W)) < 0.6).astype(np.uint8))


def _frame(gap=None):
    """200 x 200, a 3-pixel foreground frame two pixels inside the border; `gap` = list of pixels turned back to background"""
    p = np.zeros((200, 200), np.uint8)
    p[2:198, 2:198] = 1
    p[5:195, 5:195] = 0
    for (y, x) in (gap or ()):
        p[y, x] = 0
    return p


# a one-pixel-wide cut through the 3-pixel frame (rows / columns 2..4 resp. 195..197)
FRAME_GAPS = {
    'top': [(2, 100), (3, 100), (4, 100)],
    'bottom': [(195, 77), (196, 77), (197, 77)],
    'left': [(90, 2), (90, 3), (90, 4)],
    'right': [(150, 195), (150, 196), (150, 197)],
    # through the top side at column 64, then on along row 5..: the cut's pixels are the first column of the second tile column,
    # and the path from it into the interior passes the tile corner (64, 64)
    'tile_corner_column': [(2, 64), (3, 64), (4, 64)],
    # through the left side at row 128 (first row of the third tile row); columns 2..4
    'tile_corner_row': [(128, 2), (128, 3), (128, 4)],
}


def test_hole_across_tiles_is_filled(ops):
    p = _frame()
    got = _check(ops, p)
    assert got[5:195, 5:195].all() and not got[:2].any() and got.sum() == 196 * 196


@pytest.mark.parametrize('side', sorted(FRAME_GAPS))
def test_one_pixel_gap_keeps_everything(ops, side):
    p = _frame(FRAME_GAPS[side])
    got = _check(ops, p)
    assert np.array_equal(got, p)


def test_narrow_passage_through_a_tile_corner(ops):
    """background everywhere except foreground walls that leave the 2 x 2 block of pixels around the tile corner (64, 64) as the
    only way from the closed lower-right room to the rest: (63,63) (63,64) / (64,63) (64,64) are four different tiles"""
    p = np.zeros((130, 130), np.uint8)
    p[64, 65:] = 1          # the room's top wall (row 64, right of the corner pixel)
    p[65:, 63] = 1          # the room's left wall (column 63, below the corner)
    p[64, 63] = 1           # closes the diagonal: the room opens through (64, 64) -> (63, 64) only
    p[:, -1] = 1
    p[-1, :] = 1            # the room does not touch the image edge
    got = _check(ops, p)
    assert np.array_equal(got, p)
    p[63, 64] = 1           # now (64,64) touches (63,63) diagonally only: the room is a hole
    got = _check(ops, p)
    assert got[65:-1, 64:-1].all() and got[64, 64] == 1 and got[0, 0] == 0


def _serpentine(H, W, closed):
    p = np.ones((H, W), np.uint8)
    right = True
    for r in range(1, H - 1, 2):
        p[r, 1:W - 1] = 0
        if r + 2 <= H - 2:
            p[r + 1, W - 2 if right else 1] = 0
            right = not right
    if not closed:
        p[1, 0] = 0
    return p


@pytest.mark.parametrize('shape', [(129, 257), (1023, 1025)], ids=lambda s: '{}x{}'.format(*s))
@pytest.mark.parametrize('closed', [True, False], ids=['closed', 'open'])
def test_serpentine(ops, shape, closed):
    """one background corridor through every other row: the long-chain case for find"""
    p = _serpentine(*shape, closed)
    got = _check(ops, p)
    if closed:
        assert got.all()
        if shape == (129, 257):
            assert int(got.sum()) - int(p.sum()) == 16383
    else:
        assert np.array_equal(got, p)


RANDOM_SIZES = [(31, 33), (64, 64), (65, 130), (129, 257), (248, 248)]


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('dens', [0.5, 0.6, 0.7])
@pytest.mark.parametrize('shape', RANDOM_SIZES, ids=lambda s: '{}x{}'.format(*s))
def test_random(ops, shape, dens, seed):
    H, W = shape
    rng = np.random.default_rng(1000 * seed + H + W)
    p = (rng.random((H, W)) < dens).astype(np.uint8)
    want = _ref(p)
    assert (want != p).any(), 'the reference fills nothing: the case shows nothing'
    assert (want == 0).any(), 'the reference keeps no background: the case shows nothing'
    out, _ = _fill(ops, p)
    assert torch.equal(out.cpu(), torch.from_numpy(want))


def test_batch_images_are_independent(ops):
    H, W = 65, 130
    p = np.zeros((3, H, W), np.uint8)
    p[1, 10:60, 10:120] = 1
    p[1, 13:57, 13:117] = 0                                   # closed ring
    p[2] = (np.random.default_rng(5).random((H, W)) < 0.6)
    want = _ref(p)
    assert not want[0].any() and want[1, 13:57, 13:117].all() and (want[2] != p[2]).any()
    out, _ = _fill(ops, p)
    for i in range(3):
        assert torch.equal(out[i].cpu(), torch.from_numpy(want[i])), i


def test_foreground_values_and_in_place(ops):
    rng = np.random.default_rng(11)
    fg = rng.random((70, 131)) < 0.6
    p = np.where(fg, np.where(rng.random(fg.shape) < 0.5, 255, 7), 0).astype(np.uint8)
    want = torch.from_numpy(_ref(p))
    assert set(np.unique(want.numpy())) == {0, 1}
    out, _ = _fill(ops, p)
    assert torch.equal(out.cpu(), want)
    t = torch.from_numpy(p).to(DEV)
    out2, _ = ops.fill_holes(t, out=t)
    assert out2 is t and torch.equal(t.cpu(), want)


def _bincount_cm(truth, filled, ignore):
    keep = (truth != ignore) & (truth < 2)
    return np.bincount(truth[keep].astype(np.int64) * 2 + filled[keep], minlength=4).reshape(2, 2)


def test_fused_histogram(ops):
    rng = np.random.default_rng(3)
    N, H, W = 2, 67, 150
    p = (rng.random((N, H, W)) < 0.6).astype(np.uint8)
    truth = (rng.random((N, H, W)) < 0.4).astype(np.uint8)
    truth[rng.random((N, H, W)) < 0.1] = 255
    filled = _ref(p)
    want = _bincount_cm(truth, filled, 255)
    assert want.min() > 0
    td = torch.from_numpy(truth).to(DEV)
    out, cm = _fill(ops, p, truth=td, ignore_index=255)
    assert torch.equal(out.cpu(), torch.from_numpy(filled))
    assert cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), want)
    # a second call accumulates; ignore_index=None counts every truth < 2 (255 is dropped by the class range alone)
    _, cm2 = _fill(ops, p, truth=td, ignore_index=None, cm=cm)
    assert cm2 is cm and np.array_equal(cm.cpu().numpy(), 2 * want)
    # the C entry point without an output map: only the histogram
    from cutmix_semisup_seg_amd import _lib
    pd = torch.from_numpy(p).to(DEV)
    cm3 = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    nbytes = _lib.fn['cms_fill_holes_workspace_bytes'](N, H, W)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    _lib.check(_lib.fn['cms_fill_holes'](pd.data_ptr(), None, td.data_ptr(), 255, cm3.data_ptr(), N, H, W, ws.data_ptr(),
                                         nbytes, torch.cuda.current_stream().cuda_stream), 'cms_fill_holes')
    assert np.array_equal(cm3.cpu().numpy(), want)
    # ops.fill_holes with out=None allocates the map
    out4, cm4 = ops.fill_holes(pd, out=None, truth=td, ignore_index=255)
    assert torch.equal(out4.cpu(), torch.from_numpy(filled)) and np.array_equal(cm4.cpu().numpy(), want)


@pytest.mark.parametrize('align', [True, False], ids=['align', 'noalign'])
def test_evaluator_fills_on_the_device(ops, monkeypatch, align):
    """EvaluatorIoU(2, fill_holes=True): sample_logits, sample on a 2-D pair and sample on an (N,H,W) pair, with scipy's
    binary_fill_holes made to raise while the evaluator runs. The reference is built from argmax_confusion's own map, so float
    ties of the argmax are no part of this test."""
    from cutmix_semisup_seg_amd.evaluation import EvaluatorIoU
    N, H, W = 3, 248, 248
    g = torch.Generator().manual_seed(17)
    logits = torch.randn(N, 2, 62, 62, generator=g).to(DEV)
    truth = (torch.rand(N, H, W, generator=g) < 0.4).to(torch.uint8)
    truth[:, 100:110, :] = 255
    _, pred = ops.argmax_confusion(logits, None, 2, (H, W), align_corners=align, want_pred=True)
    pred_h = pred.cpu().numpy()
    filled = _ref(pred_h)
    assert (filled != pred_h).any() and (filled == 0).any()
    want = _bincount_cm(truth.numpy(), filled, 255).astype(np.float64)
    want_i = np.diag(want)
    want_u = want.sum(axis=0) + want.sum(axis=1) - want_i

    def refuse(*a, **k):
        raise AssertionError('scipy.ndimage.binary_fill_holes reached: hole filling left the device')
    monkeypatch.setattr(ndimage, 'binary_fill_holes', refuse)
    import scipy.ndimage
    assert scipy.ndimage.binary_fill_holes is refuse

    def check(ev, k):
        assert np.array_equal(ev.cm, k * want)
        assert np.array_equal(ev.intersection, k * want_i) and np.array_equal(ev.union, k * want_u)
        assert np.array_equal(ev.score(), want_i / np.maximum(want_u, 1.0))

    ev = EvaluatorIoU(2, True)
    ev.sample_logits(logits, truth.to(DEV)[:, None], ignore_value=255, align_corners=align)
    check(ev, 1)
    ev.sample_logits(logits, truth.to(DEV), out_size=(H, W), ignore_value=255, align_corners=align)
    check(ev, 2)

    ev = EvaluatorIoU(2, True)
    for i in range(N):
        ev.sample(truth[i].numpy(), pred_h[i], 255)           # numpy 2-D pairs: one image each
    check(ev, 1)
    ev.sample(truth.numpy(), pred_h.astype(np.int64), 255)    # one (N,H,W) pair: N independent images
    check(ev, 2)
    ev.sample(truth.to(DEV), pred, 255)                       # device tensors; the caller's prediction map is left alone
    check(ev, 3)
    assert torch.equal(pred.cpu(), torch.from_numpy(pred_h))
