"""
CPU-only: CowMask without a GPU.

  * the two restatements of the definition (tests/_cowmask_refs.py: explicit zero-padded passes, scipy's gaussian_filter) agree
  * mask_gen.CowMaskGenerator: the draw order of the host scalars, the tap table, the refusals
  * the two new ABI symbols: declared, exported, prototyped, version 101; every CMS_EINVAL case (decided before any HIP call)
  * the command line of train_seg_semisup_cowmask_mt: the CutMix trainer's with --boxmask_* replaced in place by --cow_sigma_range
  * csrc/cowmask_math.hpp -- the functions the kernels of csrc/cowmask.hip are made of -- driven on the host by a small program of
    its own (tests/hostcheck_cowmask) over every pixel of the GPU test's cases, against the oracle; and the same
    stand-alone program once more under the host's address and undefined-behaviour sanitizers
"""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO
import _hostcheck
import _cowmask_refs as R



# ------------------------------------------------------------------------------------------------------------------ oracle
@pytest.fixture(scope='module')
def oracle():
    """case -> (inputs, mask, stats, margin), computed once"""
    out = {}
    for ci in R.CASES:
        inp = R.case_inputs(ci)
        out[ci] = (inp,) + R.cowmask(inp['noise'], inp['taps'], inp['factor'])
    return out


@pytest.mark.parametrize('ci', sorted(R.CASES))
def test_the_two_oracle_routes_agree(ci):
    inp = R.case_inputs(ci)
    a = R.smooth(inp['noise'], inp['taps'])
    b = R.smooth_scipy(inp['noise'], inp['sigma'], inp['radius'])
    err = float(np.abs(a - b).max())
    print('case', ci, 'radius', inp['radius'], 'max |explicit - scipy| =', err)
    assert err <= 1e-14


def test_case_radii_and_margins(oracle):
    assert oracle[0][0]['radius'] == 24 and oracle[3][0]['radius'] == 64
    assert oracle[1][0]['radius'] > 9                                      # R > H
    for ci, (inp, mask, stats, margin) in oracle.items():
        print('case', ci, 'min |s - tau| =', margin, 'share of ones', mask.mean(axis=(1, 2, 3)), 'p', inp['p'])
        assert margin >= 1e-9
        assert np.abs(mask.mean(axis=(1, 2, 3)) - inp['p']).max() < 0.1       # "about p": a smooth field is not a normal sample


# ------------------------------------------------------------------------------------------------------------------ generator
def test_generate_scalars_draw_order():
    from cutmix_semisup_seg_amd import mask_gen
    g = mask_gen.CowMaskGenerator((0.2, 0.8), (4.0, 16.0))
    p, sigma = g.generate_scalars(7, rng=np.random.RandomState(42))
    rng = np.random.RandomState(42)
    want_p = rng.uniform(0.2, 0.8, size=(7,))
    want_sigma = np.exp(rng.uniform(np.log(4.0), np.log(16.0), size=(7,)))
    assert p.dtype == np.float64 and sigma.dtype == np.float64
    assert np.array_equal(p, want_p) and np.array_equal(sigma, want_sigma)
    params = g.generate_params(7, (33, 65), rng=np.random.RandomState(42))
    assert params.shape == (7, 2) and np.array_equal(params[:, 0], want_p) and np.array_equal(params[:, 1], want_sigma)
    # nothing else is drawn: the stream is where two uniform draws leave it
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    g.generate_params(3, (8, 8), rng=r1)
    r2.uniform(size=(3,)), r2.uniform(size=(3,))
    assert r1.uniform() == r2.uniform()


def test_kernel_table_is_gaussian_kernels():
    from cutmix_semisup_seg_amd import mask_gen
    g = mask_gen.CowMaskGenerator((0.2, 0.8), (4.0, 16.0))
    sigma = np.array([4.0, 7.5, 16.0])
    taps, radius = g.kernel_table(sigma)
    assert radius == 64 and taps.shape == (3, 129) and taps.dtype == np.float64
    assert np.array_equal(taps, mask_gen.gaussian_kernels(sigma, max_sigma=16.0, truncate=4.0))
    assert np.abs(taps.sum(axis=1) - 1.0).max() < 1e-15
    assert mask_gen.CowMaskGenerator(0.5, 3).kernel_table(np.array([3.0]))[1] == 12       # one number is lo = hi
    f = g.threshold_factors(np.array([0.0, 0.5, 0.975, 1.0]))
    assert f[0] == 0.0 and f[1] == 0.0 and f[3] == 0.0 and abs(f[2] - 1.959963984540054) < 1e-12


def test_generator_refusals_come_before_the_gpu(monkeypatch):
    import torch
    from cutmix_semisup_seg_amd import mask_gen

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(torch.cuda, 'is_available', no_gpu)
    monkeypatch.setattr(torch.cuda, 'current_device', no_gpu)
    for sigma_range in ((0.0, 4.0), (-1.0, 4.0), (5.0, 4.0)):
        with pytest.raises(ValueError, match='sigma_range'):
            mask_gen.CowMaskGenerator((0.2, 0.8), sigma_range)
    with pytest.raises(ValueError, match='radius'):
        mask_gen.CowMaskGenerator((0.2, 0.8), (4.0, 32.2))                 # R = 129
    assert mask_gen.CowMaskGenerator((0.2, 0.8), (4.0, 32.0)).radius == 128
    for prop_range in ((-0.1, 0.5), (0.2, 1.1), (0.8, 0.2)):
        with pytest.raises(ValueError, match='prop_range'):
            mask_gen.CowMaskGenerator(prop_range, (4.0, 16.0))
    assert mask_gen.CowMaskGenerator((0.0, 1.0), (4.0, 16.0)).prop_range == (0.0, 1.0)


def test_ops_refuse_cpu_tensors():
    import torch
    from cutmix_semisup_seg_amd import ops
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.cowmask(torch.zeros(1, 1, 4, 4), np.ones((1, 1)), np.zeros(1))


def test_the_package_does_not_import_scipy():
    code = ('import sys; sys.path.insert(0, {!r}); import cutmix_semisup_seg_amd.mask_gen, cutmix_semisup_seg_amd.ops, '
            'cutmix_semisup_seg_amd.train_seg_semisup_cowmask_mt; '
            'assert not any(m == "scipy" or m.startswith("scipy.") for m in sys.modules)').format(REPO)
    import sys
    subprocess.check_call([sys.executable, '-c', code])


# ------------------------------------------------------------------------------------------------------------------ ABI
NAMES = ('cms_cowmask_workspace_bytes', 'cms_cowmask')


def test_symbols_are_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bsize_t\s+cms_cowmask_workspace_bytes\s*\(int n, int h, int w\);', header)
    assert re.search(r'\bint\s+cms_cowmask\s*\(const float\* noise, const double\* taps, const double\* thresh_factor, int n, int h, '
                     r'int w, int radius,\s*float\* mask_out, double\* stats_out, void\* workspace, size_t workspace_bytes, '
                     r'void\* stream\);', header)
    for name in NAMES:
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_cowmask_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    res, args = _lib.PROTOTYPES['cms_cowmask']
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_workspace_bytes():
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_cowmask_workspace_bytes']
    # two fp64 planes and two fp64 per tile of the second pass (32 along x, 64 along y)
    assert f(1, 1, 1) == (2 + 2) * 8
    assert f(3, 37, 53) == (2 * 3 * 37 * 53 + 2 * 3 * 2 * 1) * 8
    assert f(4, 512, 1024) == (2 * 4 * 512 * 1024 + 2 * 4 * 32 * 8) * 8
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (2, 2 ** 15, 2 ** 15), (2 ** 16, 1, 1)):
        assert f(*bad) == 0, bad


def test_bad_arguments_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_cowmask']
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = ctypes.c_size_t(2 ** 40)
    #        noise taps factor n  h  w  radius mask stats ws   ws_bytes
    good = (p, p, p, 1, 4, 4, 2, p, None, p, big)
    bad = []
    for i in (0, 1, 2, 7, 9):                                       # NULL pointers (stats_out may be NULL)
        bad.append(good[:i] + (None,) + good[i + 1:])
    for i, v in ((3, 0), (3, -1), (4, 0), (4, -3), (5, 0), (5, -1), (6, -1), (6, 129), (6, 2 ** 31 - 1)):
        bad.append(good[:i] + (v,) + good[i + 1:])
    bad.append(good[:3] + (2, 2 ** 15, 2 ** 15) + good[6:])         # 2^31 pixels
    bad.append(good[:3] + (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) + good[6:])
    bad.append(good[:10] + (ctypes.c_size_t((2 * 16 + 2) * 8 - 1),))   # a workspace one byte short
    for args in bad:
        assert f(*args, None) == -1, args
        assert _lib.fn['cms_last_error']()
    with pytest.raises(ValueError):
        _lib.check(f(*((None,) + good[1:]), None), 'cms_cowmask')
    assert b'NULL' in _lib.fn['cms_last_error']()


# ------------------------------------------------------------------------------------------------------------------ command
def _table(command):
    return [(p.name, type(p.type).__name__, p.default, getattr(p, 'is_flag', False)) for p in command.params]


def test_option_table_is_the_cutmix_trainers_with_the_substitution():
    import train_seg_semisup_mask_mt as cutmix
    import train_seg_semisup_cowmask_mt as cow
    base = _table(cutmix.experiment)
    names = [t[0] for t in base]
    box = [n for n in names if n.startswith('boxmask_')]
    assert box == ['boxmask_n_boxes', 'boxmask_fixed_aspect_ratio', 'boxmask_by_size', 'boxmask_outside_bounds', 'boxmask_no_invert']
    at = names.index(box[0])
    assert names[at:at + 5] == box                                   # contiguous: replaced IN PLACE
    want = names[:at] + ['cow_sigma_range'] + names[at + 5:]
    got = _table(cow.experiment)
    assert [t[0] for t in got] == want
    # every shared option keeps its type and default, but for the share of ones
    by_name = dict((t[0], t) for t in base)
    for t in got:
        if t[0] == 'cow_sigma_range':
            assert t[1:] == ('StringParamType', '4:16', False)
        elif t[0] == 'mask_prop_range':
            assert t[1:] == ('StringParamType', '0.2:0.8', False)
        else:
            assert t == by_name[t[0]], t
    assert cow.train_seg_semisup_cowmask_mt is not None
    assert cutmix.experiment.params[names.index('mask_prop_range')].default == '0.5'


def test_command_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import torch
    import train_seg_semisup_cowmask_mt as cow

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(torch.cuda, 'is_available', no_gpu)
    monkeypatch.setattr(torch.cuda, 'current_device', no_gpu)
    monkeypatch.chdir(tmp_path)
    for extra, what in ((['--cow_sigma_range', '0:4'], 'sigma_range'), (['--cow_sigma_range', '4:40'], 'radius'),
                        (['--cow_sigma_range', 'wide'], 'cow_sigma_range'), (['--mask_prop_range', '0.5:1.5'], 'prop_range')):
        res = CliRunner().invoke(cow.experiment, ['--synthetic', '--crop_size', '33,33'] + extra)
        assert res.exit_code != 0 and isinstance(res.exception, ValueError), (res.output, res.exception)
        assert what in str(res.exception)


# ------------------------------------------------------------------------------------------------------------------ host driver
def _request(inp):
    """-> (header, blocks)"""
    n, h, w = inp['noise'].shape
    return struct.pack('<4i', n, h, w, inp['radius']), [(inp['taps'], np.float64), (inp['factor'], np.float64), (inp['noise'], np.float32)]


def _result(raw, inp):
    n, h, w = inp['noise'].shape
    out = _hostcheck.split(raw, [('mask', np.float32, (n, 1, h, w)), ('stats', np.float64, (n, 2))])
    return out['mask'], out['stats']


@pytest.fixture(scope='module')
def hostcheck():
    exe = _hostcheck.build('hostcheck_cowmask')

    def run(inp, program=exe, expect_code=0):
        raw = _hostcheck.run(program, *_request(inp), expect_code=expect_code)
        return None if raw is None else _result(raw, inp)
    return run


@pytest.mark.parametrize('ci', sorted(R.CASES))
def test_header_on_the_host_vs_oracle_every_pixel(hostcheck, oracle, ci):
    inp, mask, stats, margin = oracle[ci]
    got_mask, got_stats = hostcheck(inp)
    assert np.array_equal(got_mask, mask)
    assert np.all(np.abs(got_stats - stats) <= 1e-12 * (1.0 + np.abs(stats)))


def _small(n, h, w, radius, sigma, seed, p=0.5):
    rng = np.random.RandomState(seed)
    sig = np.full((n,), float(sigma))
    offs = np.arange(-radius, radius + 1, dtype=np.float64)[None]
    taps = np.exp(offs * offs * (-0.5 / (sig[:, None] ** 2)))
    taps /= taps.sum(axis=1, keepdims=True)
    return dict(noise=rng.standard_normal((n, h, w)).astype(np.float32), taps=taps, radius=radius, factor=R.factors(np.full((n,), p)))


# sizes at which the tiling takes another path: one pixel, radius 0 (no halo), the largest radius, tile edges at 32 / 64, more than one
# tile each way
SMALL = [(1, 1, 1, 0, 1.0), (1, 1, 1, 128, 9.0), (2, 5, 3, 0, 1.0), (1, 32, 64, 3, 1.0), (1, 33, 65, 4, 1.5), (1, 64, 32, 128, 30.0),
         (2, 70, 131, 7, 2.0), (1, 3, 200, 128, 20.0), (1, 200, 3, 100, 20.0)]


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s[:4])))
def test_header_on_the_host_tile_edges(hostcheck, shape):
    inp = _small(*shape, seed=sum(shape[:4]))
    mask, stats, margin = R.cowmask(inp['noise'], inp['taps'], inp['factor'])
    got_mask, got_stats = hostcheck(inp)
    assert np.all(np.abs(got_stats - stats) <= 1e-12 * (1.0 + np.abs(stats)))
    if inp['noise'][0].size > 1:                     # one pixel: s == tau up to the rounding of a zero variance
        assert margin >= 1e-12
        assert np.array_equal(got_mask, mask)
    else:
        assert got_mask.min() >= 0.0 and got_mask.max() <= 1.0


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    inp = _small(1, 4, 4, 2, 1.0, 0)
    hostcheck(dict(inp, radius=129, taps=np.zeros((1, 259))), expect_code=2)


def test_stand_alone_under_the_host_sanitizers(hostcheck, oracle):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_cowmask', sanitize=True)
    for inp, want in [(oracle[0][0], oracle[0][1]), (oracle[1][0], oracle[1][1])]:
        got_mask, _ = hostcheck(inp, program=exe)
        assert np.array_equal(got_mask, want)
    inp = _small(1, 33, 65, 128, 30.0, 3)
    got_mask, _ = hostcheck(inp, program=exe)
    assert np.array_equal(got_mask, R.cowmask(inp['noise'], inp['taps'], inp['factor'])[0])
