"""
CPU-only: the C ABI of the device hole filling (csrc/fillholes.hip). Argument validation happens before any HIP call, so every
refusal is checkable without a GPU; what the kernels compute is tests/test_gpu_fill_holes.py's business.
"""
import ctypes
import glob
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, 'include', 'cutmixseg.h')


@pytest.fixture(scope='module')
def lib():
    from cutmix_semisup_seg_amd import _lib
    return _lib


def test_entry_points_are_exported_declared_and_prototyped(lib):
    header = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in ('cms_fill_holes', 'cms_fill_holes_workspace_bytes'):
        assert hasattr(lib.lib, name), 'libcutmixseg_hip.so does not export {}'.format(name)
        assert re.search(r'\b{}\s*\('.format(name), header), '{} is not declared in cutmixseg.h'.format(name)
        assert name in lib.PROTOTYPES and name in lib.fn
    res, args = lib.PROTOTYPES['cms_fill_holes_workspace_bytes']
    assert res is ctypes.c_size_t and args == [ctypes.c_int] * 3
    res, args = lib.PROTOTYPES['cms_fill_holes']
    assert res is ctypes.c_int and len(args) == 11 and args[9] is ctypes.c_size_t
    assert lib.version() == 101


@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (1, 1, 7), (1, 7, 1), (3, 65, 130), (10, 248, 248), (1, 1023, 1025),
                                   (1, 46340, 46340), (2, 32767, 32767)])
def test_workspace_covers_one_int32_per_node(lib, n, h, w):
    nbytes = lib.fn['cms_fill_holes_workspace_bytes'](n, h, w)
    assert nbytes > 0 and nbytes >= 4 * n * (h * w + 1)
    assert nbytes < 2 * 4 * n * (h * w + 1)


@pytest.mark.parametrize('n,h,w', [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4),
                                   (1, 46341, 46341),           # h * w + 1 >= 2^31
                                   (2, 32768, 32768),           # n * (h * w + 1) >= 2^31
                                   (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)])
def test_workspace_is_zero_on_bad_geometry(lib, n, h, w):
    assert lib.fn['cms_fill_holes_workspace_bytes'](n, h, w) == 0


def test_bad_arguments_come_back_as_error_codes_not_crashes(lib):
    """every pointer below is a fake non-NULL address: a refusal must come before anything dereferences or launches"""
    f, err = lib.fn['cms_fill_holes'], lib.fn['cms_last_error']
    P, O, T, CM, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    big = 1 << 40
    cases = [
        ((None, O, None, -1, None, 1, 4, 4, WS, big, None), b'pred NULL'),
        ((P, None, None, -1, None, 1, 4, 4, WS, big, None), b'nothing to produce'),
        ((P, O, T, 255, None, 1, 4, 4, WS, big, None), b'truth given without cm'),
        ((P, None, T, 255, None, 1, 4, 4, WS, big, None), b'nothing to produce'),
        ((P, O, None, 255, CM, 1, 4, 4, WS, big, None), b'cm given without truth'),
        ((P, O, None, -1, None, 0, 4, 4, WS, big, None), b'bad geometry'),
        ((P, O, None, -1, None, 1, 0, 4, WS, big, None), b'bad geometry'),
        ((P, O, None, -1, None, 1, 4, -3, WS, big, None), b'bad geometry'),
        ((P, O, None, -1, None, 1, 46341, 46341, WS, big, None), b'2^31'),
        ((P, O, None, -1, None, 2, 32768, 32768, WS, big, None), b'2^31'),
        ((P, O, None, -1, None, 1, 4, 4, None, big, None), b'workspace too small'),
        ((P, O, None, -1, None, 1, 4, 4, WS, 4 * 17 - 1, None), b'workspace too small'),
        ((P, O, T, 255, CM, 3, 65, 130, WS, 4 * 3 * (65 * 130 + 1) - 4, None), b'workspace too small'),
    ]
    for args, text in cases:
        rc = f(*args)
        assert rc == -1, args
        assert text in err(), (args, err())
        with pytest.raises(ValueError):
            lib.check(rc, 'cms_fill_holes')


def test_ops_fill_holes_refuses_cpu_tensors_and_wrong_types():
    import torch
    from cutmix_semisup_seg_amd import ops
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.fill_holes(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.fill_holes(torch.zeros(2, 4, 4, dtype=torch.uint8), truth=torch.zeros(2, 4, 4, dtype=torch.uint8))


def test_product_package_does_not_import_scipy():
    files = sorted(glob.glob(os.path.join(REPO, 'cutmix-semisup-seg_amd', '*.py')))
    assert len(files) >= 15
    for path in files:
        src = open(path).read()
        assert not re.search(r'^\s*(import\s+scipy|from\s+scipy)', src, flags=re.M), path
        assert 'import scipy' not in src and 'from scipy' not in src, path
