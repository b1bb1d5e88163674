"""
CPU check of the staging per-pixel arithmetic the HIP kernels inline (cutmix-semisup-seg_amd/csrc/stage_math.hpp), driven on the
host over a RAGGED pool by tests/hostcheck_stage (test infrastructure: every batch sample read from its own pool entry, as
csrc/stage.hip does) and compared per sample with the numpy restatement of the reference's transforms (oracle/augment.py). The
kernels themselves are covered by tests/test_gpu_stage.py.

Tolerances: the project's own for this arithmetic (tests/test_gpu_augment.py): image 2e-4, mask 1e-5, labels exact, colour
view 2e-3.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import _hostcheck
import _stage_cases as sc


@pytest.fixture(scope='module')
def hc():
    lib = _hostcheck.load('hostcheck_stage')
    lib.hc_stage_entry_address.restype = ctypes.c_ulonglong
    lib.hc_stage_entry_address.argtypes = [ctypes.c_ulonglong, ctypes.c_longlong]
    return lib


@pytest.fixture(scope='module')
def pool():
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    images, labels = sc.make_pool_arrays()
    return ResidentPool(ArraySource(images, labels), range(len(images)), 'cpu'), images, labels


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def run_host(hc, pool, index, params, crop, with_labels, colour):
    """DeviceAugmenter.stage on the host: luminance pre-pass, pivot, image pass -- over the pool's own buffers and table."""
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    n, (H, W) = len(index), crop
    img, lab, table = pool.image_buffer.numpy(), pool.label_buffer.numpy(), np.ascontiguousarray(pool.table)
    idx = pool.entries_of(index)
    p = np.ascontiguousarray(params, dtype=np.float32).copy()
    mean, std = sc.MEAN.astype(np.float32), sc.STD.astype(np.float32)
    if colour:
        luma = np.zeros(n, dtype=np.float32)
        hc.hc_stage_luma(_ptr(img), _ptr(table), len(table), _ptr(idx), n, H, W, _ptr(p), _ptr(luma))
        p[:, 14] = luma * DeviceAugmenter._pivot_scale(params)
    out0 = np.zeros((n, 3, H, W), dtype=np.float32)
    out1 = np.zeros_like(out0) if colour else None
    labs = np.zeros((n, H, W), dtype=np.uint8) if with_labels else None
    mask = np.zeros((n, H, W), dtype=np.float32)
    hc.hc_stage_batch(_ptr(img), _ptr(lab) if with_labels else None, _ptr(table), len(table), _ptr(idx), n, H, W, _ptr(p),
                      _ptr(mean), _ptr(std), _ptr(out0), _ptr(out1), _ptr(labs), _ptr(mask))
    return dict(image=out0, image_stu=out1, labels=labs, mask=mask)


@pytest.mark.parametrize('name', list(sc.CONFIGS))
def test_ragged_staging_arithmetic_vs_oracle(hc, pool, name):
    rp, images, labels = pool
    aug, crop, with_labels, cfg = sc.make_augmenter(name)
    params = aug.draw_params(len(sc.INDEX), rp.sizes_of(sc.INDEX), with_labels=with_labels)
    sc.assert_branches_covered(name, params)
    out = run_host(hc, rp, sc.INDEX, params, crop, with_labels, bool(cfg.get('strong_colour')))
    worst = sc.compare_with_oracle(name, params, images, labels, out)
    print('{}: largest differences image {:.3g}, mask {:.3g}, colour view {:.3g}'.format(name, *worst))
    if cfg.get('strong_colour'):
        same = [i for i in range(len(sc.INDEX)) if not params[i, 12] and not params[i, 11]]
        assert same and all(np.array_equal(out['image'][i], out['image_stu'][i]) for i in same)
    # the same entry staged twice (batch rows 2 and 3) went through different parameters
    assert not np.array_equal(params[2], params[3]) or not cfg


def test_pool_sizes_cover_the_edge_cases():
    sizes = sc.POOL_SIZES
    assert (1, 1) in sizes and (48, 64) in sizes
    assert any(h < 48 and w >= 64 for h, w in sizes) and any(h >= 48 and w < 64 for h, w in sizes)
    assert any(h < 48 and w < 64 for h, w in sizes)
    assert any((3 * w) % 2 == 1 for _, w in sizes)                                   # rows at odd byte offsets
    assert len(set(sc.INDEX)) < len(sc.INDEX) and sc.INDEX != sorted(sc.INDEX) and set(sc.INDEX) == set(range(len(sizes)))


def test_eval_canvas_arithmetic(hc, pool):
    """stage_eval's parameters (window mode, negative origin, scale 1) on the host: the standardised image inside each rectangle,
    exactly 0 / 255 outside."""
    from cutmix_semisup_seg_amd.datapipe.seg_data import collate_geometry
    rp, images, labels = pool
    index = [4, 3, 6, 1]
    (hc_, wc), offsets = collate_geometry(rp.sizes_of(index), (32, 32))
    assert (hc_, wc) == (96, 96)
    params = np.zeros((len(index), 24), dtype=np.float32)
    for i, (top, left) in enumerate(offsets):
        params[i, 0:4] = (-top, -left, hc_, wc)
    out = run_host(hc, rp, index, params, (hc_, wc), True, False)
    for i, e in enumerate(index):
        h, w = sc.POOL_SIZES[e]
        top, left = offsets[i]
        want = ((images[e].astype(np.float64) / 255.0 - sc.MEAN) / sc.STD).transpose(2, 0, 1)
        np.testing.assert_allclose(out['image'][i][:, top:top + h, left:left + w], want, rtol=1e-5, atol=1e-5)
        assert np.array_equal(out['labels'][i][top:top + h, left:left + w], labels[e])
        outside = np.ones((hc_, wc), dtype=bool)
        outside[top:top + h, left:left + w] = False
        assert (out['image'][i][:, outside] == 0).all() and (out['labels'][i][outside] == 255).all()
        assert (out['mask'][i][outside] == 0).all() and (out['mask'][i][~outside] == 1).all()


def test_entry_address_is_64_bit(hc):
    """The byte address of an entry whose offset lies above 2^32 (address arithmetic only; no memory is touched)."""
    base = 0x7f0000000000
    for off in (0, 16, (1 << 32) + 16, (5 << 32) + 48, (1 << 33) - 16, 7 * 10 ** 9):
        assert hc.hc_stage_entry_address(base, off) == base + off


def test_unusable_index_or_entry_stages_as_an_empty_source(hc, pool):
    rp, images, labels = pool
    H, W = 8, 8
    table = np.ascontiguousarray(rp.table)
    for bad in (-1, len(table), 10 ** 6):
        idx = np.array([bad], dtype=np.int32)
        p = np.zeros((1, 24), dtype=np.float32)
        p[0, 2:4] = (H, W)
        out0 = np.full((1, 3, H, W), 9.0, dtype=np.float32)
        labs = np.zeros((1, H, W), dtype=np.uint8)
        mask = np.ones((1, H, W), dtype=np.float32)
        mean, std = sc.MEAN.astype(np.float32), sc.STD.astype(np.float32)
        hc.hc_stage_batch(_ptr(rp.image_buffer.numpy()), _ptr(rp.label_buffer.numpy()), _ptr(table), len(table), _ptr(idx), 1, H, W,
                          _ptr(p), _ptr(mean), _ptr(std), _ptr(out0), None, _ptr(labs), _ptr(mask))
        assert (out0 == 0).all() and (labs == 255).all() and (mask == 0).all()


def test_stand_alone_under_the_host_sanitizers():
    """The checker behind its own main, built with -fsanitize=address,undefined, as a process of its own: it draws its own small
    inputs and ends non-zero on a non-finite result or a sanitizer report."""
    assert subprocess.call([_hostcheck.build('hostcheck_stage', sanitize=True)]) == 0
