"""
CPU-only: the Cityscapes converter without a GPU.

  * csrc/convert_math.hpp -- the functions the kernels of csrc/convert.hip are made of -- driven on the host by a small program
    of its own (tests/hostcheck_convert), against the numpy restatement of the reference's arithmetic
    (tests/_convert_refs.py): every possible block sum for d = 1..8, the vote with its ties, word and byte paths, short groups
  * the two new ABI symbols: declared, exported, prototyped, version 101; every CMS_EINVAL case (decided before any HIP call)
  * every refusal of the converter's command line, with the GPU booby-trapped
"""
import ctypes
import os
import struct

import numpy as np
import pytest

from conftest import REPO
import _hostcheck
import _convert_refs as R
import _zip_archives as Z


@pytest.fixture(scope='module')
def hostcheck():
    """the host driver, compiled with the host C++ compiler -> run(kind, x, d, in_off, out_off) -> output array"""
    exe = _hostcheck.build('hostcheck_convert')

    def run(x, d_, in_off=0, out_off=0, expect_code=0):
        x = np.ascontiguousarray(x, dtype=np.uint8)
        kind = 0 if x.ndim == 4 else 1
        n, h, w = x.shape[:3]
        raw = _hostcheck.run(exe, struct.pack('<7i', kind, n, h, w, d_, in_off, out_off), [(x, np.uint8)], expect_code)
        if raw is None:
            return None
        shape = (n, h // d_, w // d_) + ((3,) if kind == 0 else ())
        return _hostcheck.split(raw, [('out', np.uint8, shape)])['out']
    return run


@pytest.mark.parametrize('d', range(1, 9))
def test_block_mean_is_the_truncated_float64_mean_for_every_sum(hostcheck, d):
    img = R.sums_image(d)[None]
    want = R.block_mean_u8(img, d)
    assert want.shape == (1, 1, 255 * d * d + 1, 3)
    assert np.array_equal(want[0, 0, :, 0], np.arange(255 * d * d + 1) // (d * d))        # ... which is floor(sum / d^2)
    for in_off, out_off in ((0, 0), (1, 3)):
        assert np.array_equal(hostcheck(img, d, in_off, out_off), want)


IMAGE_SHAPES = [(1, 2, 2, 2), (1, 3, 3, 3), (2, 8, 8, 8), (1, 6, 390, 2), (3, 14, 518, 7), (1, 5, 7, 1), (2, 4, 32, 2), (2, 8, 40, 4),
                (1, 10, 45, 5), (1, 12, 54, 6)]


@pytest.mark.parametrize('shape', IMAGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_image_groups_vs_numpy(hostcheck, shape):
    n, h, w, d = shape
    rng = np.random.RandomState(sum(shape))
    noise = rng.randint(0, 256, size=(n, h, w, 3))
    channels = np.broadcast_to(np.array([11, 130, 251]), (n, h, w, 3))
    edge, base = R.floor_not_round_image(rng, n, h, w, d)
    assert np.array_equal(R.block_mean_u8(edge, d), base)
    for x in (noise, np.full((n, h, w, 3), 255), channels, edge):
        want = R.block_mean_u8(x.astype(np.uint8), d)
        for in_off, out_off in ((0, 0), (2, 1)):
            assert np.array_equal(hostcheck(x, d, in_off, out_off), want)


def test_vote_ties_by_hand_and_vs_numpy(hostcheck):
    y, want = R.hand_made_ties()
    assert np.array_equal(R.block_vote(y, 2), want)            # the restatement agrees with the hand count
    assert np.array_equal(hostcheck(y, 2), want) and np.array_equal(hostcheck(y, 2, 3, 1), want)


LABEL_SHAPES = [(1, 2, 2, 2), (2, 6, 390, 2), (2, 4, 32, 2), (1, 3, 3, 3), (3, 14, 518, 7), (2, 8, 8, 8), (1, 5, 7, 1), (1, 16, 40, 8),
                (2, 8, 44, 4), (1, 10, 45, 5), (1, 12, 54, 6), (1, 9, 48, 3)]


@pytest.mark.parametrize('shape', LABEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_groups_vs_numpy(hostcheck, shape):
    n, h, w, d = shape
    rng = np.random.RandomState(sum(shape) + 1)
    for hi in (34, 2, 256):
        y = rng.randint(0, hi, size=(n, h, w)).astype(np.uint8)
        want = R.block_vote(y, d)
        for in_off, out_off in ((0, 0), (1, 2)):
            assert np.array_equal(hostcheck(y, d, in_off, out_off), want)
    if d == 2:
        two = rng.randint(0, 2, size=(4, 32, 64)).astype(np.uint8)
        ties = (two.reshape(4, 16, 2, 32, 2).sum(axis=(2, 4)) == 2).mean()
        assert ties >= 0.25, ties                               # 2-2 ties are 6/16 of random blocks
    if d == 8:
        distinct, lowest = R.distinct_blocks(rng)
        assert np.array_equal(R.block_vote(distinct, 8), lowest)
        assert np.array_equal(hostcheck(distinct, 8), lowest)


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    hostcheck(np.zeros((1, 4, 6), dtype=np.uint8), 4, expect_code=2)
    hostcheck(np.zeros((1, 18, 18), dtype=np.uint8), 9, expect_code=2)


# ------------------------------------------------------------------------------------------------------------------ ABI
NAMES = ('cms_downsample_image_u8', 'cms_downsample_labels_u8')


def test_symbols_are_declared_exported_and_prototyped():
    import re
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r'\bint\s+{}\s*\(const uint8_t\* src, int n, int h, int w, int d, uint8_t\* dst, void\* stream\);'.format(name),
                         header), name
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and args == [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


@pytest.mark.parametrize('name', NAMES)
def test_bad_arguments_return_einval_before_any_hip_call(name):
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn[name]
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    c = 3 if 'image' in name else 1
    bad = [(None, 1, 4, 4, 2, p), (p, 1, 4, 4, 2, None),                       # NULL pointers
           (p, 0, 4, 4, 2, p), (p, -1, 4, 4, 2, p), (p, 1, 0, 4, 2, p), (p, 1, 4, -4, 2, p),
           (p, 1, 4, 4, 0, p), (p, 1, 4, 4, -2, p), (p, 1, 18, 18, 9, p),    # d outside 1..8
           (p, 1, 6, 4, 4, p), (p, 1, 4, 6, 4, p), (p, 1, 3, 3, 2, p),       # not divisible
           (p, 2 ** 31 - 1, 2, 2, 2, p), (p, 1, 2 ** 16, 2 ** 16, 2, p), (p, 2, 2 ** 15, 2 ** 15, 1, p),   # > 2^31 - 1 bytes
           (p, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1, p)]
    if c == 3:
        bad.append((p, 1, 2 ** 15, 2 ** 15, 1, p))                                 # 3 * 2^30 bytes of image, 2^30 of labels
    for src, n, h, w, d, dst in bad:
        assert f(src, n, h, w, d, dst, None) == -1, (n, h, w, d)
        assert _lib.fn['cms_last_error']()
    with pytest.raises(ValueError):
        _lib.check(f(None, 1, 4, 4, 2, p, None), name)
    assert b'NULL' in _lib.fn['cms_last_error']()


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from cutmix_semisup_seg_amd import ops
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.downsample_image_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.downsample_labels_u8(torch.zeros(1, 4, 4, dtype=torch.uint8), 2)


# ------------------------------------------------------------------------------------------------------------------ converter
def test_names_are_derived_as_the_reference_derives_them():
    from cutmix_semisup_seg_amd import convert_cityscapes as cc
    names = ['leftImg8bit/', 'leftImg8bit/train/aachen/aachen_000000_000019_leftImg8bit.png', 'README',
             'leftImg8bit/test/berlin/berlin_000000_000019_leftImg8bit.png', 'leftImg8bit/val/lindau/lindau_000000_000019_leftImg8bit.PNG']
    assert cc.members_to_process(names) == [
        (names[1], 'gtFine/train/aachen/aachen_000000_000019_gtFine_labelIds.png', 'train/aachen/aachen_000000_000019'),
        (names[4], 'gtFine/val/lindau/lindau_000000_000019_gtFine_labelIds.png', 'val/lindau/lindau_000000_000019')]
    # chunks: consecutive samples of one size, bounded by bytes, never empty
    sizes = [(4, 8)] * 5 + [(2, 8)] + [(4, 8)] * 2
    assert cc.plan_chunks(sizes, 4 * 8 * 4 * 2) == [(0, 2), (2, 4), (4, 5), (5, 6), (6, 8)]
    assert cc.plan_chunks(sizes, 1) == [(i, i + 1) for i in range(8)]
    assert cc.plan_chunks(sizes, 1 << 30) == [(0, 5), (5, 6), (6, 8)]


def test_converter_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import torch
    import convert_cityscapes as prog

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(torch.cuda, 'is_available', no_gpu)
    monkeypatch.setattr(torch.cuda, 'current_device', no_gpu)
    monkeypatch.chdir(tmp_path)
    left, gt, out = str(tmp_path / 'left.zip'), str(tmp_path / 'gt.zip'), tmp_path / 'made' / 'here' / 'cityscapes.zip'
    names = [n for n, _ in Z.CITYSCAPES[:3]]
    Z.write_official_cityscapes(left, gt, names, size=(6, 8))

    def run(*args):
        res = CliRunner().invoke(prog.convert, list(args))
        assert res.exit_code != 0 and not isinstance(res.exception, AssertionError), (res.output, res.exception)
        assert not out.exists()
        return res.output + str(res.exception)

    # no configuration, then a configuration without the key
    assert 'cityscapes' in run(left, gt) and 'semantic_segmentation.cfg' in run(left, gt)
    Z.write_config(str(tmp_path), camvid='/nowhere.zip')
    assert 'cityscapes' in run(left, gt)
    Z.write_config(str(tmp_path), cityscapes=str(out))
    for d in ('0', '-1', '9'):
        assert '1..8' in run(left, gt, '--downsample', d)
    assert '--downsample 4 does not divide' in run(left, gt, '--downsample', '4')          # 6 x 8
    assert 'does not divide' in run(left, gt, '--downsample', '3')                           # 8 columns
    assert 'does not exist' in run(str(tmp_path / 'missing.zip'), gt)
    # an image whose label map is missing, and one whose label map has another size
    Z.write_official_cityscapes(str(tmp_path / 'unused.zip'), str(tmp_path / 'gt_short.zip'), names[:2], size=(6, 8))
    assert 'has no label map' in run(left, str(tmp_path / 'gt_short.zip'))
    Z.write_official_cityscapes(str(tmp_path / 'left_big.zip'), str(tmp_path / 'unused.zip'), names, size=(12, 8))
    assert 'but its label map' in run(str(tmp_path / 'left_big.zip'), gt)
    import zipfile
    with zipfile.ZipFile(str(tmp_path / 'empty.zip'), 'w') as z:
        z.writestr('leftImg8bit/test/berlin/berlin_000000_000019_leftImg8bit.png', b'')
    assert 'holds no' in run(str(tmp_path / 'empty.zip'), gt)
    defaults = {p.name: p.default for p in prog.convert.params}
    assert defaults['downsample'] == 2
