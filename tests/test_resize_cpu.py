"""
CPU-only: the ISIC 2017 converter without a GPU.

  * csrc/resize_math.hpp -- the functions the kernels of csrc/resize.hip are made of -- driven on the host by a small program of
    its own (tests/hostcheck_resize), against the numpy restatement (tests/_resize_refs.py): the weight properties for
    every 1 <= Lo <= L <= 40, the rounded division for every numerator at seven denominators, the image cases on the word and the
    byte path, the statistics
  * the two new ABI symbols: declared, exported, prototyped, version 101; every CMS_EINVAL case (decided before any HIP call)
  * every refusal of the converter's command line, with the GPU booby-trapped, and its pure helpers
"""
import ctypes
import os
import struct

import numpy as np
import pytest

from conftest import REPO
import _hostcheck
import _resize_refs as R
import _isic_archives as A
import _zip_archives as Z


@pytest.fixture(scope='module')
def hostcheck():
    """the host driver, compiled with the host C++ compiler -> run(kind, args, payload) -> the result file's bytes"""
    exe = _hostcheck.build('hostcheck_resize')

    def run(kind, args, payload=b'', expect_code=0):
        args = list(args) + [0] * (8 - len(args))
        return _hostcheck.run(exe, struct.pack('<9i', kind, *args) + payload, expect_code=expect_code)
    return run


def host_resize(hostcheck, x, ho, wo, in_off=0, out_off=0):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n, h, w = x.shape[:3]
    c = 3 if x.ndim == 4 else 1
    out = hostcheck(2, [n, h, w, c, ho, wo, in_off, out_off], x.tobytes())
    return np.frombuffer(out, dtype=np.uint8).reshape((n, ho, wo) + ((3,) if c == 3 else ()))


def test_weight_properties_for_every_pair_of_sizes_up_to_40(hostcheck):
    for L in range(1, 41):
        for Lo in range(1, L + 1):
            out = np.frombuffer(hostcheck(0, [L, Lo]), dtype=np.int32)
            wt, first, end = out[:Lo * L].reshape(Lo, L), out[Lo * L:Lo * L + Lo], out[Lo * L + Lo:]
            assert np.array_equal(wt, R.weight_matrix(L, Lo)), (L, Lo)
            assert (wt.sum(axis=1) == L).all() and (wt.sum(axis=0) == Lo).all(), (L, Lo)
            assert ((wt > 0).sum(axis=0) <= 2).all(), (L, Lo)
            for o in range(Lo):                                 # the cell bounds are exactly the pixels with weight
                assert np.array_equal(np.flatnonzero(wt[o]), np.arange(first[o], end[o])), (L, Lo, o)
                assert end[o] - first[o] <= -(-L // Lo) + 1


@pytest.mark.parametrize('den', [1, 2, 3, 4, 6, 24, 35])
def test_rounded_division_ties_to_even_for_every_numerator(hostcheck, den):
    got = np.frombuffer(hostcheck(1, [den]), dtype=np.int64)
    want = []
    for num in range(255 * den + 1):                            # Python integers
        q, r = divmod(num, den)
        want.append(q + 1 if 2 * r > den else q + (q & 1) if 2 * r == den else q)
    assert got.tolist() == want
    assert np.array_equal(R.round_half_even_div(np.arange(255 * den + 1), den), got)      # ... and the restatement's division
    if den % 2 == 0:
        assert [want[k * den + den // 2] for k in range(4)] == [0, 2, 2, 4]


@pytest.mark.parametrize('case', R.SMALL_CASES + [R.FRAME_CASE, R.BIG_NUMERATOR_CASE], ids=R.case_id)
def test_work_items_vs_numpy(hostcheck, case):
    n, h, w, c, ho, wo = case
    for name, x in R.case_inputs(case).items():
        want = R.case_want(case, name)
        if name == 'white':
            assert (want == 255).all()
        if name == 'channels':
            assert (want == np.array([11, 130, 251])).all()
        for in_off, out_off in ((0, 0), (1, 3)):
            assert np.array_equal(host_resize(hostcheck, x, ho, wo, in_off, out_off), want), (name, in_off)


def test_the_specific_inputs_are_what_they_claim(hostcheck):
    """on the restatement alone: every output of the tie image is an exact half with both parities of k, and the bright image's
    numerators pass 2^32; the host program rounds those halves to the even value"""
    rng = np.random.RandomState(4)
    x, k = R.tie_image(rng)
    assert R.is_tie(x, 2, 3).mean() == 1.0
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    assert np.array_equal(R.area_resize_u8(x, 2, 3), k + k % 2)
    assert np.array_equal(host_resize(hostcheck, x, 2, 3), k + k % 2)
    case = (2, 4, 6, 3, 2, 3)
    assert R.is_tie(R.case_inputs(case)['ties'], 2, 3).mean() == 1.0
    n, h, w, c, ho, wo = R.BIG_NUMERATOR_CASE
    for name, x in R.case_inputs(R.BIG_NUMERATOR_CASE).items():
        assert R.numerators(x, ho, wo).max() > 2 ** 32, name


def test_statistics_vs_numpy(hostcheck):
    rng = np.random.RandomState(8)
    for shape in ((3, 5, 7, 3), (2, 31, 29, 3), (1, 1, 1), (2, 300, 3)):
        for x in (rng.randint(0, 256, size=shape).astype(np.uint8), np.full(shape, 255, dtype=np.uint8)):
            c = 3 if x.ndim == 4 else 1
            got = np.frombuffer(hostcheck(3, [shape[0], shape[1] * shape[2], c], x.tobytes()), dtype=np.int64).reshape(shape[0], 2 * c)
            assert np.array_equal(got, R.sum_sumsq(x))
    # the float64 formula of the converter against the reference's accumulation
    from cutmix_semisup_seg_amd import convert_isic as ci
    imgs = [rng.randint(0, 256, size=(9, 11, 3)).astype(np.uint8), rng.randint(0, 256, size=(5, 4, 3)).astype(np.uint8)]
    s = sum(R.sum_sumsq(i[None])[0] for i in imgs)
    mean, std = ci.mean_std_from_sums([int(v) for v in s[:3]], [int(v) for v in s[3:]], 9 * 11 + 5 * 4)
    ref_mean, ref_std = R.mean_std(imgs)
    assert mean.dtype == np.float64 and std.dtype == np.float64 and mean.shape == (3,) and std.shape == (3,)
    assert np.allclose(mean, ref_mean, rtol=1e-9, atol=0) and np.allclose(std, ref_std, rtol=1e-9, atol=0)


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    z = bytes(4 * 6 * 3)
    hostcheck(2, [1, 4, 6, 3, 5, 6, 0, 0], z, expect_code=2)            # ho > h
    hostcheck(2, [1, 4, 6, 3, 4, 7, 0, 0], z, expect_code=2)            # wo > w
    hostcheck(2, [1, 4, 6, 2, 2, 3, 0, 0], z, expect_code=2)            # c = 2
    hostcheck(2, [1, 4, 6, 3, 0, 3, 0, 0], z, expect_code=2)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_prototyped():
    import re
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+cms_resize_area_u8\s*\(const uint8_t\* src, int n, int h, int w, int c, int ho, int wo, uint8_t\* dst, '
                     r'void\* stream\);', header)
    assert re.search(r'\bint\s+cms_sum_sumsq_u8\s*\(const uint8_t\* src, int n, int pixels, int c, int64_t\* sums, void\* stream\);', header)
    want = {'cms_resize_area_u8': [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2,
            'cms_sum_sumsq_u8': [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2}
    for name, args in want.items():
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
        assert _lib.PROTOTYPES[name] == (ctypes.c_int, args)
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_bad_arguments_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = _lib.fn['cms_resize_area_u8']
    bad = [(None, 1, 4, 4, 3, 2, 2, p), (p, 1, 4, 4, 3, 2, 2, None),                               # NULL pointers
           (p, 1, 4, 4, 2, 2, 2, p), (p, 1, 4, 4, 0, 2, 2, p), (p, 1, 4, 4, 4, 2, 2, p), (p, 1, 4, 4, -1, 2, 2, p),      # c
           (p, 0, 4, 4, 3, 2, 2, p), (p, -1, 4, 4, 3, 2, 2, p), (p, 1, 0, 4, 3, 2, 2, p), (p, 1, 4, -4, 3, 2, 2, p),
           (p, 1, 4, 4, 3, 0, 2, p), (p, 1, 4, 4, 3, 2, 0, p), (p, 1, 4, 4, 1, -2, 2, p),                    # a non-positive size
           (p, 1, 4, 4, 3, 5, 4, p), (p, 1, 4, 4, 1, 4, 5, p),                                               # enlarging
           (p, 1, 16385, 4, 1, 2, 2, p), (p, 1, 4, 16385, 3, 2, 2, p),                                       # a side above 16384
           (p, 2 ** 31 - 1, 2, 2, 1, 1, 1, p), (p, 8, 16384, 16384, 1, 2, 2, p), (p, 2 ** 17, 128, 128, 1, 1, 1, p),
           (p, 3, 16384, 16384, 3, 2, 2, p), (p, 2 ** 31 - 1, 16384, 16384, 3, 1, 1, p)]                 # > 2^31 - 1 bytes
    for src, n, h, w, c, ho, wo, dst in bad:
        assert f(src, n, h, w, c, ho, wo, dst, None) == -1, (n, h, w, c, ho, wo)
        assert _lib.fn['cms_last_error']()
    with pytest.raises(ValueError):
        _lib.check(f(None, 1, 4, 4, 3, 2, 2, p, None), 'cms_resize_area_u8')
    assert b'NULL' in _lib.fn['cms_last_error']()
    f = _lib.fn['cms_sum_sumsq_u8']
    bad = [(None, 1, 4, 3, p), (p, 1, 4, 3, None), (p, 1, 4, 2, p), (p, 1, 4, 0, p), (p, 1, 4, 4, p), (p, 0, 4, 3, p), (p, -1, 4, 1, p),
           (p, 1, 0, 3, p), (p, 1, -4, 1, p), (p, 2 ** 16, 2 ** 15, 1, p), (p, 1, 2 ** 30, 3, p), (p, 2 ** 31 - 1, 2 ** 31 - 1, 3, p)]
    for src, n, pixels, c, sums in bad:
        assert f(src, n, pixels, c, sums, None) == -1, (n, pixels, c)
        assert _lib.fn['cms_last_error']()
    with pytest.raises(ValueError):
        _lib.check(f(p, 1, 4, 3, None, None), 'cms_sum_sumsq_u8')
    assert b'NULL' in _lib.fn['cms_last_error']()


def test_ops_refuse_cpu_tensors():
    import torch
    from cutmix_semisup_seg_amd import ops
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.resize_area_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 2, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.resize_area_u8(torch.zeros(1, 4, 4, dtype=torch.uint8), 2, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sum_sumsq_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ converter
def test_pure_helpers():
    from cutmix_semisup_seg_amd import convert_isic as ci
    names = ['ISIC-2017_Training_Data/', 'ISIC-2017_Training_Data/ISIC_0000000.jpg', 'ISIC-2017_Training_Data/ISIC_0000000_superpixels.png',
             'ISIC-2017_Training_Data/ISIC_0000001_superpixels.jpg', 'ISIC-2017_Training_Data/ISIC_0000002_SuperPixels.JPG',
             'ISIC-2017_Training_Data/ISIC_0000003.JPG', 'ISIC-2017_Training_Data/ISIC-2017_Training_Data_metadata.csv',
             'ISIC-2017_Training_Data/ISIC_0000001.jpg']
    assert ci.members_to_process(names, 'GT', 'train') == [
        (names[1], 'GT/ISIC_0000000_segmentation.png', 'train/ISIC_0000000'),
        (names[5], 'GT/ISIC_0000003_segmentation.png', 'train/ISIC_0000003'),
        (names[7], 'GT/ISIC_0000001_segmentation.png', 'train/ISIC_0000001')]
    # the three option forms
    assert ci.parse_out_size('248,248') == (248, 248) and ci.parse_out_size(' 72 , 96 ') == (72, 96)
    assert ci.parse_out_size('65') == 65 and ci.parse_out_size(' 65 ') == 65
    assert ci.parse_out_size('') is None and ci.parse_out_size('  ') is None
    for bad in ('a', '1,2,3', '0', '-5', '0,8', '8,-1', '7.5', ','):
        with pytest.raises(SystemExit, match='out_size'):
            ci.parse_out_size(bad)
    # output sizes: fixed, none, and the shorter side with Python's round (halves to even)
    assert ci.target_size(767, 1022, (248, 248)) == (248, 248) and ci.target_size(767, 1022, None) == (767, 1022)
    assert ci.target_size(96, 128, 65) == (65, 87) and ci.target_size(131, 97, 65) == (88, 65)
    assert 120 * 65 / 80 == 97.5 and ci.target_size(80, 120, 65) == (65, 98)            # a half goes to the even size ...
    assert 44 * 5 / 8 == 27.5 and ci.target_size(8, 44, 5) == (5, 28) and 20 * 5 / 8 == 12.5 and ci.target_size(20, 8, 5) == (12, 5)
    # chunks: consecutive samples, bounded by bytes, never empty, sizes mixed
    sizes = [(4, 8)] * 3 + [(2, 8)] * 2 + [(8, 8)]
    assert ci.plan_chunks(sizes, 4 * 8 * 4 * 2) == [(0, 2), (2, 5), (5, 6)]
    assert ci.plan_chunks(sizes, 4 * 8 * 4 * 2 - 1) == [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6)]
    assert ci.plan_chunks(sizes, 1) == [(i, i + 1) for i in range(6)]
    assert ci.plan_chunks(sizes, 1 << 30) == [(0, 6)]
    assert ci.plan_chunks([], 1 << 30) == []
    assert ci.same_size_runs(sizes) == [(0, 3), (3, 5), (5, 6)] and ci.same_size_runs([]) == []
    assert ci.DEFAULT_CHUNK_BYTES == 1 << 30


def test_converter_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import shutil
    import torch
    import convert_isic as prog

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(torch.cuda, 'is_available', no_gpu)
    monkeypatch.setattr(torch.cuda, 'current_device', no_gpu)
    monkeypatch.chdir(tmp_path)
    zips, out = str(tmp_path / 'zips'), tmp_path / 'made' / 'here' / 'isic2017.zip'
    A.write_official_isic(zips)

    def run(*args):
        res = CliRunner().invoke(prog.convert_isic, list(args))
        assert res.exit_code != 0 and not isinstance(res.exception, AssertionError), (res.output, res.exception)
        assert not out.exists()
        return res.output + str(res.exception)

    # no configuration, then a configuration without the key
    assert 'isic2017' in run(zips) and 'semantic_segmentation.cfg' in run(zips)
    Z.write_config(str(tmp_path), camvid='/nowhere.zip')
    assert 'isic2017' in run(zips)
    Z.write_config(str(tmp_path), isic2017=str(out))
    for bad in ('a,b', '1,2,3', '0', '-3,4', 'x'):
        assert '--out_size must be' in run(zips, '--out_size', bad)
    # a target larger than a source along either axis: 80 rows, 97 columns are the smallest
    assert 'larger than the source' in run(zips, '--out_size', '81,90') and '.jpg is 80x120' in run(zips, '--out_size', '81,90')
    assert 'larger than the source' in run(zips, '--out_size', '72,98') and '.JPG is 131x97' in run(zips, '--out_size', '72,98')
    assert 'larger than the source' in run(zips, '--out_size', '97')                   # the shorter side of 96 x 128 would grow
    # a missing archive, named
    for name in ('ISIC-2017_Training_Data.zip', 'ISIC-2017_Validation_Part1_GroundTruth.zip'):
        short = str(tmp_path / ('without_' + name))
        shutil.copytree(zips, short)
        os.remove(os.path.join(short, name))
        text = run(short)
        assert 'does not exist' in text and name in text
    assert 'does not exist' in run(str(tmp_path / 'nowhere'))
    # no .jpg members
    import zipfile
    empty = str(tmp_path / 'empty')
    shutil.copytree(zips, empty)
    with zipfile.ZipFile(os.path.join(empty, 'ISIC-2017_Validation_Data.zip'), 'w') as z:
        z.writestr('ISIC-2017_Validation_Data/ISIC_0001769_superpixels.jpg', b'')
        z.writestr('ISIC-2017_Validation_Data/ISIC_0001769_superpixels.png', b'')
    text = run(empty)
    assert 'holds no .jpg members' in text and 'ISIC-2017_Validation_Data.zip' in text
    # an image whose mask is missing, and one whose mask has another size
    A.write_official_isic(str(tmp_path / 'no_mask'), skip_mask_of='ISIC_0012086')
    text = run(str(tmp_path / 'no_mask'))
    assert 'has no mask' in text and 'ISIC_0012086_segmentation.png' in text
    A.write_official_isic(str(tmp_path / 'other_size'), mask_size_of=('ISIC_0001960', (90, 90)))
    text = run(str(tmp_path / 'other_size'), '--out_size', '72,72')
    assert 'but its mask' in text and 'ISIC_0001960' in text and '90x90' in text
    defaults = {p.name: p.default for p in prog.convert_isic.params}
    assert defaults['out_size'] == '248,248'
