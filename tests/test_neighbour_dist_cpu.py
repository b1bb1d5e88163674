"""
CPU-only: what the neighbouring-patch distance maps (cutmix-semisup-seg_amd/patch_dist.py: neighbouring_patch_distance_maps,
patch_average_distance_map, box_sum) promise before a GPU is touched. The C ABI of the new entry points, box_sum against goldens
the reference's own patch_dist.py wrote (tests/golden/make_neighbour_dist_golden.py), the refusals, and the test-side brute force
(tests/_neighbour_dist_refs.py) against the same goldens: the GPU tests hold the device to that brute force.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
import _neighbour_dist_refs as R

HEADER = os.path.join(REPO, 'include', 'cutmixseg.h')
NEW_SYMBOLS = ('cms_pd_box_sum', 'cms_pd_neighbour_workspace_bytes', 'cms_pd_neighbour_maps')
CASES = [('img_a', (3, 3)), ('img_a', (5, 3)), ('img_a', (15, 15)), ('img_b', (7, 7)), ('img_c', (5, 5))]


def case_key(name, shape):
    return '{}_p{}x{}'.format(name, shape[0], shape[1])


@pytest.fixture(scope='module')
def G():
    return load_golden('neighbour_dist')


def _no_gpu(monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(torch.cuda, 'is_available', touched)
    monkeypatch.setattr(torch.cuda, 'current_device', touched)


def test_entry_points_are_exported_declared_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(_lib.lib, name), 'libcutmixseg_hip.so does not export {}'.format(name)
        assert re.search(r'\b{}\s*\('.format(name), header), '{} is not declared in cutmixseg.h'.format(name)
        assert name in _lib.PROTOTYPES and name in _lib.fn
    assert _lib.version() == 101


def test_bad_arguments_come_back_as_error_codes_not_crashes():
    """every pointer is a fake non-NULL address: a refusal must come before anything dereferences or launches"""
    from cutmix_semisup_seg_amd import _lib
    f, err = _lib.fn, _lib.fn['cms_last_error']
    A, B, Cc = 0x1000, 0x2000, 0x3000
    entry = _lib.StageEntry(0, -1, 10, 12)
    nb, box, by = f['cms_pd_neighbour_maps'], f['cms_pd_box_sum'], f['cms_pd_neighbour_workspace_bytes']
    for ph, pw in ((4, 5), (5, 8), (0, 3), (3, -1), (-3, 3)):
        assert nb(A, ctypes.byref(entry), ph, pw, B, Cc, None) == -1 and b'odd' in err(), (ph, pw)
        assert by(10, 12, ph, pw) == 0
    for args in ((None, ctypes.byref(entry), 3, 3, B, Cc), (A, None, 3, 3, B, Cc), (A, ctypes.byref(entry), 3, 3, None, Cc),
                 (A, ctypes.byref(entry), 3, 3, B, None)):
        assert nb(*(args + (None,))) == -1 and b'NULL' in err()
    assert nb(A, ctypes.byref(_lib.StageEntry(0, -1, 0, 12)), 3, 3, B, Cc, None) == -1 and b'bad pool entry' in err()
    assert nb(A, ctypes.byref(_lib.StageEntry(0, -1, 40000, 40000)), 3, 3, B, Cc, None) == -1 and b'2^30' in err()
    for args in ((None, 0, 4, 4, 1, 1, B, Cc), (A, 0, 4, 4, 1, 1, None, Cc), (A, 1, 4, 4, 1, 1, B, None)):
        assert box(*(args + (None,))) == -1 and b'NULL' in err()
    for hp, wp, ph, pw in ((4, 4, 0, 1), (4, 4, 1, -1), (4, 4, 5, 1), (4, 4, 1, 5), (0, 4, 1, 1), (1 << 15, 1 << 15, 3, 3)):
        assert box(A, 0, hp, wp, ph, pw, B, Cc, None) == -1 and b'box' in err(), (hp, wp, ph, pw)
    # the workspace: the box sums' int64 intermediate plane and the two int32 planes of squared differences
    hs, ws, ph, pw = 10, 12, 5, 3
    hp, wp = hs + ph - 1, ws + pw - 1
    need = 8 * max(hs * (wp + 1), (hs + 1) * wp) + 4 * hp * (wp + 1) + 4 * (hp + 1) * wp
    assert need <= by(hs, ws, ph, pw) <= need + 48


@pytest.mark.parametrize('kind', ['int', 'float'])
def test_box_sum_equals_the_reference(G, kind):
    import patch_dist
    if kind == 'int':
        got = patch_dist.box_sum(G['box_int_plane'], (5, 3))
        assert got.dtype == np.int64 and got.shape == (5, 11)
        assert np.array_equal(got, G['box_int_sum'])
        assert np.array_equal(got, R.brute_box_sum(G['box_int_plane'], (5, 3)))
        # an integer input stays an integer whatever its width: exact where float64 would round
        big = np.full((4, 4), 2 ** 53 + 1, dtype=np.int64)
        assert patch_dist.box_sum(big, (1, 1))[0, 0] == 2 ** 53 + 1
        small = patch_dist.box_sum(np.full((6, 7), 200, dtype=np.uint8), (6, 7))
        assert small.dtype.kind in 'iu' and small.shape == (1, 1) and int(small[0, 0]) == 200 * 42
    else:
        got = patch_dist.box_sum(G['box_float_plane'], (3, 5))
        assert got.dtype == np.float64 and got.shape == G['box_float_sum'].shape == (9, 10)
        np.testing.assert_allclose(got, G['box_float_sum'], rtol=1e-12, atol=0)


def test_float_images_are_a_type_error_before_the_gpu(monkeypatch):
    import patch_dist
    _no_gpu(monkeypatch)
    for fn in (patch_dist.neighbouring_patch_distance_maps, patch_dist.patch_average_distance_map):
        with pytest.raises(TypeError, match='img_as_float'):
            fn(np.zeros((8, 8, 3)), (3, 3))
        with pytest.raises(TypeError, match='uint8'):
            fn(np.zeros((8, 8, 3), dtype=np.float32), (3, 3))


def test_even_patch_sizes_are_a_value_error_before_the_gpu(monkeypatch):
    import patch_dist
    _no_gpu(monkeypatch)
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for fn in (patch_dist.neighbouring_patch_distance_maps, patch_dist.patch_average_distance_map):
        for bad in ((4, 5), (5, 8), (0, 3)):
            with pytest.raises(ValueError, match='odd'):
                fn(img, bad)
    with pytest.raises(ValueError, match='odd'):
        patch_dist.neighbour_sqr_distance_maps(None, 0, (6, 6))             # before the pool is looked at


def test_the_drop_in_module_resolves_the_reference_names():
    import patch_dist
    from cutmix_semisup_seg_amd import patch_dist as impl
    for name in ('neighbouring_patch_distance_maps', 'patch_average_distance_map', 'box_sum', 'neighbour_sqr_distance_maps'):
        assert getattr(patch_dist, name) is getattr(impl, name)
    assert not re.search(r'^\s*(import|from)\s+scipy', open(impl.__file__).read(), flags=re.M)
    assert np.array_equal(patch_dist.NEIGHBOUR_OFFSETS, np.array(R.OFFSETS))


@pytest.mark.parametrize('name,shape', CASES)
def test_brute_force_agrees_with_the_reference_goldens(G, name, shape):
    """np.rint(g^2 * 65025) == D2 where the reference is finite, D2 == 0 where it is NaN. The margin of 1/2 is a condition; the
    reference's own error against it, stored by the golden script, is below 1e-6 at these sizes."""
    key = case_key(name, shape)
    maps, image = G[key + '_maps'], G[name]
    d2 = R.brute_neighbour_d2(image, shape)
    assert d2.dtype == np.int64 and d2.shape == maps.shape == (4,) + image.shape[:2]
    ok, err = R.golden_agrees(maps, d2)
    print('{}: worst |g^2 * 65025 - D2| {:.3e} (stored {:.3e}), NaNs {}, exact zeros {}'.format(
        key, err, float(G[key + '_ref_err']), int(np.isnan(maps).sum()), int((d2 == 0).sum())))
    assert ok
    assert err < 1e-6
    nans = int(np.isnan(maps).sum())
    if name == 'img_c':
        assert 0 < nans < int((d2 == 0).sum())                 # zeros the reference turned into NaN, and zeros it kept
    else:
        assert nans == 0
    # the two identities the device may use, on the brute force itself
    assert np.array_equal(d2[1][:, :-1], d2[0][:, 1:]) and np.array_equal(d2[3][:-1], d2[2][1:])
    # the average in the reference's order, from the exact maps
    m = [np.sqrt(d2[k].astype(np.float64)) / 255.0 for k in range(4)]
    avg = (m[0] + m[1] + m[2] + m[3]) * 0.25
    fin = np.isfinite(G[key + '_avg'])
    assert np.array_equal(fin, np.isfinite(maps).all(axis=0))
    # |g^2 * 65025 - D2| <= e bounds |g - sqrt(D2) / 255| by sqrt(e) / 255 where D2 == 0 and by e / 255 where D2 >= 1
    np.testing.assert_allclose(avg[fin], G[key + '_avg'][fin], rtol=0, atol=np.sqrt(err) / 255.0 + 1e-15)


def test_torch_restatement_equals_the_brute_force():
    import torch
    rng = np.random.RandomState(11)
    for (h, w), shape in (((2, 3), (5, 3)), ((7, 9), (3, 7)), ((1, 1), (3, 3)), ((6, 5), (15, 1))):
        image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        got = R.torch_neighbour_d2(torch.from_numpy(image), shape)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), R.brute_neighbour_d2(image, shape)), ((h, w), shape)
