"""
GPU: the neighbouring-patch distance maps on the device (csrc/patchdist.hip: pd_neighbour_squares, pd_box_columns, pd_box_rows;
patch_dist.neighbour_sqr_distance_maps and the reference drop-ins on top of it).

  exact D2     torch.equal against the int64 brute force (tests/_neighbour_dist_refs.py). All arithmetic is on integers, so there is
               no tolerance. Before each call the output is filled with -1 and the workspace with 0x7f bytes: neither may have to
               be initialised, and every element of the output must be written
  box sum      ops.pd_box_sum alone against numpy, on int32 and int64 planes
  goldens      the reference's own float64 maps: np.rint(g^2 * 65025) == D2 where they are finite (a margin of 1/2, a condition:
               the reference's own error, stored with the goldens, is below 1e-6 at these sizes), D2 == 0 where they are NaN
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import _neighbour_dist_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _pd():
    from cutmix_semisup_seg_amd import patch_dist
    return patch_dist


def _pool(images):
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    return ResidentPool(ArraySource(images), range(len(images)), DEV, with_labels=False)


def _entry(pool, sample_i):
    from cutmix_semisup_seg_amd import _lib
    t = pool.table[int(pool.entries_of([sample_i])[0])]
    return _lib.StageEntry(int(t['img_off']), int(t['lab_off']), int(t['hs']), int(t['ws']))


@functools.lru_cache(maxsize=None)
def _image(kind, h, w):
    if kind == 'stripes':                                                    # columns alternating 0 / 255: every horizontal
        image = np.zeros((h, w, 3), dtype=np.uint8)                          # neighbour difference is 3 * 255^2
        image[:, 1::2] = 255
    else:
        image = np.random.RandomState(1000 * h + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    image.setflags(write=False)
    return image


@functools.lru_cache(maxsize=None)
def _brute(kind, h, w, shape):
    d2 = R.brute_neighbour_d2(_image(kind, h, w), shape)
    d2.setflags(write=False)
    return d2


def _device_d2(pool, sample_i, shape):
    """the four maps through ops.pd_neighbour_maps with a poisoned output and workspace"""
    from cutmix_semisup_seg_amd import ops
    entry = _entry(pool, sample_i)
    out = torch.full((4 * entry.hs * entry.ws,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((ops.pd_neighbour_workspace(entry.hs, entry.ws, shape),), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV)
    got = ops.pd_neighbour_maps(pool.image_buffer, entry, shape, out=out, work=work)
    assert got.dtype == torch.int64 and tuple(got.shape) == (4, entry.hs, entry.ws) and got.data_ptr() == out.data_ptr()
    return got


EXACT = [('noise', 1, 1, (1, 1)), ('noise', 1, 1, (3, 3)),
         ('noise', 2, 3, (5, 3)), ('noise', 2, 3, (15, 15)),                 # more than one reflection
         ('noise', 7, 9, (1, 1)), ('noise', 7, 9, (3, 7)), ('noise', 7, 9, (7, 3)),
         ('noise', 33, 40, (7, 7)), ('noise', 33, 40, (31, 31)),
         ('noise', 64, 70, (15, 15)),                                        # more than one wave wide
         ('noise', 5, 300, (3, 225)),                                        # a window longer than any per-wave segment of a row
         ('noise', 300, 5, (225, 3)),                                        # ... and than any per-thread segment of a column
         ('stripes', 16, 16, (159, 159))]                                    # the largest sum passes 2^32


@pytest.mark.parametrize('kind,h,w,shape', EXACT)
def test_d2_equals_the_brute_force(kind, h, w, shape):
    want = torch.from_numpy(_brute(kind, h, w, shape).copy())
    got = _device_d2(_pool([_image(kind, h, w)]), 0, shape).cpu()
    print('{} {} x {} patch {}: max D2 {}'.format(kind, h, w, shape, int(want.max())))
    assert int(want.min()) >= 0
    if kind == 'stripes':
        assert int(want.max()) > 1 << 32                                     # no 32-bit accumulator passes
        assert int(want[2:].max()) == 0                                      # rows are equal: up and down are 0 everywhere
    assert torch.equal(got, want)


def test_d2_of_an_entry_in_the_middle_of_a_pool():
    """entry 1 of three: a non-zero img_off, rows of 27 and 15 bytes around and in it"""
    images = [_image('noise', 7, 9), _image('noise', 12, 5), _image('noise', 9, 7)]
    pool = _pool(images)
    assert int(pool.table['img_off'][int(pool.entries_of([1])[0])]) > 0
    for shape in ((5, 3), (3, 3)):
        got = _device_d2(pool, 1, shape).cpu()
        assert torch.equal(got, torch.from_numpy(_brute('noise', 12, 5, shape).copy()))
    got = _pd().neighbour_sqr_distance_maps(pool, 2, (3, 5))
    assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(_brute('noise', 9, 7, (3, 5)).copy()))


def test_two_calls_agree_and_right_is_left_shifted():
    pool = _pool([_image('noise', 33, 40)])
    a = _device_d2(pool, 0, (7, 7))
    b = _device_d2(pool, 0, (7, 7))
    assert torch.equal(a, b)
    assert torch.equal(a[1][:, :-1], a[0][:, 1:])
    assert torch.equal(a[3][:-1], a[2][1:])


def test_even_sizes_are_an_error_code_and_write_nothing():
    from cutmix_semisup_seg_amd import _lib, ops
    pool = _pool([_image('noise', 7, 9)])
    entry = _entry(pool, 0)
    out = torch.full((4 * 7 * 9,), -1, dtype=torch.int64, device=DEV)
    work = torch.zeros((ops.pd_neighbour_workspace(7, 9, (5, 5)),), dtype=torch.int64, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ph, pw in ((4, 5), (5, 2), (0, 3)):
        rc = _lib.fn['cms_pd_neighbour_maps'](ctypes.c_void_p(pool.image_buffer.data_ptr()), ctypes.byref(entry), ph, pw,
                                              ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(out.data_ptr()), stream)
        assert rc == -1 and b'odd' in _lib.fn['cms_last_error']()
        with pytest.raises(ValueError, match='odd'):
            ops.pd_neighbour_maps(pool.image_buffer, entry, (ph, pw), out=out, work=work)
    torch.cuda.synchronize()
    assert bool((out == -1).all())


# ------------------------------------------------------------------------------------------------------------ box sum alone
BOXES = [((1, 1), (1, 1)), ((5, 7), (5, 7)), ((9, 300), (3, 225)), ((300, 9), (225, 3)), ((70, 130), (7, 5))]


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('plane,box', BOXES)
def test_box_sum_equals_numpy(plane, box, dtype):
    from cutmix_semisup_seg_amd import ops
    rng = np.random.RandomState(plane[0] * 1000 + plane[1])
    if dtype == torch.int32:
        x = rng.randint(-2 ** 31, 2 ** 31, size=plane, dtype=np.int64).astype(np.int32)      # sums far outside 32 bits
    else:
        x = rng.randint(-2 ** 40, 2 ** 40, size=plane, dtype=np.int64)
    ho, wo = plane[0] - box[0] + 1, plane[1] - box[1] + 1
    out = torch.full((ho * wo,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((ho * plane[1],), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV)
    got = ops.pd_box_sum(torch.from_numpy(x).to(DEV), box, out=out, work=work)
    assert got.dtype == torch.int64 and tuple(got.shape) == (ho, wo)
    s = np.pad(np.cumsum(np.cumsum(x.astype(np.int64), axis=1), axis=0), [[1, 0], [1, 0]])
    want = s[box[0]:, box[1]:] - s[:-box[0], box[1]:] - s[box[0]:, :-box[1]] + s[:-box[0], :-box[1]]
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(ops.pd_box_sum(torch.from_numpy(x).to(DEV), box).cpu(), torch.from_numpy(want))     # buffers of its own


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_box_sum_of_a_plane_of_the_largest_squared_difference(dtype):
    from cutmix_semisup_seg_amd import ops
    x = torch.full((70, 130), 3 * 255 * 255, dtype=dtype, device=DEV)
    for box in ((7, 5), (70, 130), (1, 130), (70, 1)):
        got = ops.pd_box_sum(x, box)
        assert tuple(got.shape) == (70 - box[0] + 1, 130 - box[1] + 1)
        assert bool((got == 195075 * box[0] * box[1]).all())
    with pytest.raises(ValueError):
        ops.pd_box_sum(x, (71, 1))
    with pytest.raises(TypeError):
        ops.pd_box_sum(x.to(torch.float32), (3, 3))


# ------------------------------------------------------------------------------------------------------------------ goldens
GOLDEN_CASES = [('img_a', (3, 3)), ('img_a', (5, 3)), ('img_a', (15, 15)), ('img_b', (7, 7)), ('img_c', (5, 5))]


@pytest.mark.parametrize('name,shape', GOLDEN_CASES)
def test_maps_match_the_reference_goldens(name, shape):
    pd = _pd()
    G = load_golden('neighbour_dist')
    key = '{}_p{}x{}'.format(name, shape[0], shape[1])
    image, maps = G[name], G[key + '_maps']
    d2 = pd.neighbour_sqr_distance_maps(_pool([image]), 0, shape).cpu().numpy()
    ok, err = R.golden_agrees(maps, d2)
    print('{}: worst |g^2 * 65025 - D2| {:.3e} (the reference against the brute force: {:.3e}), NaNs {}, exact zeros {}'.format(
        key, err, float(G[key + '_ref_err']), int(np.isnan(maps).sum()), int((d2 == 0).sum())))
    assert np.array_equal(np.rint(maps[np.isfinite(maps)] ** 2 * 65025.0), d2[np.isfinite(maps)].astype(np.float64))
    assert (d2[np.isnan(maps)] == 0).all()
    assert ok
    # the drop-ins: exactly sqrt(D2) / 255, and the average in the reference's order
    got = pd.neighbouring_patch_distance_maps(image, shape)
    assert isinstance(got, tuple) and len(got) == 4
    want = [np.sqrt(d2[k].astype(np.float64)) / 255.0 for k in range(4)]
    for k in range(4):
        assert got[k].dtype == np.float64 and got[k].shape == image.shape[:2] and np.array_equal(got[k], want[k])
    avg = pd.patch_average_distance_map(image, shape)
    assert avg.dtype == np.float64 and np.array_equal(avg, (want[0] + want[1] + want[2] + want[3]) * 0.25)
    if name == 'img_c':
        assert np.isnan(maps).any() and not np.isnan(avg).any()
        assert (np.stack(got)[np.isnan(maps)] == 0.0).all()                  # 0.0 where the reference gave NaN
