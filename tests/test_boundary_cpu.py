"""
CPU-only: the boundary scores (Boundary IoU, trimap IoU) without a GPU.

  * the two new ABI symbols: declared, exported, prototyped, version 101; the descriptor's layout in C; the workspace sizes;
    every CMS_EINVAL case (decided before any HIP call), with its message
  * ops.boundary_confusion's refusals; evaluation.parse_boundary_widths, good and bad; EvaluatorBoundary's constructor
  * eval_seg refusing a malformed --boundary_width before the GPU (and before the model file is opened)
  * the reference itself (tests/_boundary_refs.py): padding cancels, the band is the distance map thresholded
  * csrc/boundary_math.hpp -- the functions the kernels of csrc/boundary.hip are made of -- driven on the host by a small program of
    its own (tests/hostcheck_boundary) over every pixel of the GPU test's cases, against the scipy erosion reference;
    and the same stand-alone program once more under the host's address and undefined-behaviour sanitizers
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
import _boundary_refs as R



# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bsize_t\s+cms_boundary_workspace_bytes\s*\(int n, int h, int w\);', header)
    assert re.search(r'\bint\s+cms_boundary_confusion\s*\(const cms_boundary_desc\* d, void\* stream\);', header)
    for name in ('cms_boundary_workspace_bytes', 'cms_boundary_confusion'):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_boundary_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _lib.PROTOTYPES['cms_boundary_confusion'] == (ctypes.c_int, [ctypes.POINTER(_lib.BoundaryDesc), ctypes.c_void_p])
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    fields = [name for name, _ in _lib.BoundaryDesc._fields_]
    assert fields == ['truth', 'pred', 'widths', 'n', 'h', 'w', 'num_classes', 'ignore_index', 'k', 'bcm', 'tcm', 'dist_truth',
                      'dist_pred', 'workspace', 'workspace_bytes']
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu", sizeof(cms_boundary_desc));\n'
            + ''.join('printf(" %zu", offsetof(cms_boundary_desc, {}));\n'.format(f) for f in fields) + 'return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.BoundaryDesc
    assert sizes == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


def test_workspace_bytes():
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_boundary_workspace_bytes']
    # a 32-bit word per pixel from the row pass, then the two uint8 distance maps, each part rounded up to 16 bytes
    assert f(1, 1, 1) == 16 + 2 * 16
    assert f(3, 33, 41) == 16240 + 2 * 4064                                 # 4059 pixels
    assert f(10, 321, 321) == 4121640 + 8 + 2 * 1030416                     # 1030410
    assert f(4, 512, 1024) == 6 * 4 * 512 * 1024
    assert f(70000, 1, 1) == 6 * 70000                                      # no limit on the samples but the pixel count
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (-2, 4, 4), (2, 2 ** 15, 2 ** 15), (2 ** 31 - 1,) * 3):
        assert f(*bad) == 0, bad
    assert f(1, 2 ** 15, 2 ** 16 - 1) > 0 and f(1, 2 ** 15, 2 ** 16) == 0     # 2^31 - 2^15 pixels, 2^31 pixels


def _desc(**over):
    """a descriptor cms_boundary_confusion would accept (host pointers: never dereferenced before the launch), then `over`"""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    d = _lib.BoundaryDesc()
    d.truth, d.pred, d.widths, d.bcm, d.tcm, d.dist_truth, d.dist_pred, d.workspace = (p,) * 8
    d.n, d.h, d.w, d.num_classes, d.ignore_index, d.k = 1, 4, 4, 3, 255, 2
    d.workspace_bytes = 2 ** 40
    d._keep = buf
    for key, val in over.items():
        setattr(d, key, val)
    return d


BAD = [
    ('truth NULL', dict(truth=None)), ('pred NULL', dict(pred=None)), ('workspace NULL', dict(workspace=None)),
    ('widths NULL', dict(widths=None)), ('widths NULL', dict(widths=None, bcm=None)), ('widths NULL', dict(widths=None, tcm=None)),
    ('nothing to produce', dict(bcm=None, tcm=None, dist_truth=None, dist_pred=None)),
    ('k <= 4', dict(k=0)), ('k <= 4', dict(k=5)), ('k <= 4', dict(k=-1)),
    ('num_classes', dict(num_classes=0)), ('num_classes', dict(num_classes=65)), ('num_classes', dict(num_classes=-3)),
    ('geometry', dict(n=0)), ('geometry', dict(n=-1)), ('geometry', dict(h=0)), ('geometry', dict(w=-2)),
    ('2^31', dict(n=2, h=2 ** 15, w=2 ** 15)), ('2^31', dict(n=1, h=2 ** 31 - 1, w=2 ** 31 - 1)),
    ('workspace too small', dict(workspace_bytes=6 * 16 - 1)), ('workspace too small', dict(workspace_bytes=0)),
]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_boundary_confusion']
    assert f(None, None) == -1 and b'NULL descriptor' in _lib.fn['cms_last_error']()
    for what, over in BAD:
        d = _desc(**over)
        assert f(ctypes.byref(d), None) == -1, over
        assert what.encode() in _lib.fn['cms_last_error'](), (over, _lib.fn['cms_last_error']())
        assert _lib.fn['cms_last_error']().startswith(b'boundary_confusion: ')
    d = _desc()
    d.workspace = d.workspace + 8
    assert f(ctypes.byref(d), None) == -1 and b'aligned' in _lib.fn['cms_last_error']()
    with pytest.raises(ValueError, match='boundary'):
        _lib.check(f(ctypes.byref(_desc(k=9)), None), 'cms_boundary_confusion')
    # (that bcm, tcm, widths and the distance outputs may be NULL in the combinations left is tests/test_gpu_boundary.py's to show:
    # an accepted descriptor launches)


def test_ops_check_their_arguments_before_the_library():
    import torch
    from cutmix_semisup_seg_amd import ops
    t = torch.zeros(2, 8, 9, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.boundary_confusion(t, t, 3, [1, 2])
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.boundary_confusion(t[0], t[0], 3, np.array([[254]]), want_dist=True)
    for exc, call in (
            (TypeError, lambda: ops.boundary_confusion(t.long(), t, 3, [1])),
            (TypeError, lambda: ops.boundary_confusion(t, t.float(), 3, [1])),
            (TypeError, lambda: ops.boundary_confusion(t.numpy(), t, 3, [1])),
            (ValueError, lambda: ops.boundary_confusion(t, t[:, :, :8], 3, [1])),
            (ValueError, lambda: ops.boundary_confusion(t, t[0], 3, [1])),
            (ValueError, lambda: ops.boundary_confusion(t[None], t[None], 3, [1])),
            (ValueError, lambda: ops.boundary_confusion(t[:0], t[:0], 3, [1])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 0, [1])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 65, [1])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 3, [0])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 3, [1, 255])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 3, [-4])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 3, [1, 2, 3, 4, 5])),
            (ValueError, lambda: ops.boundary_confusion(t, t, 3, np.ones((3, 2), dtype=np.int64))),
            (TypeError, lambda: ops.boundary_confusion(t, t, 3, [])),
            (TypeError, lambda: ops.boundary_confusion(t, t, 3, [1.5])),
            (TypeError, lambda: ops.boundary_confusion(t, t, 3, [1], bcm=torch.zeros(1, 4, 4))),
            (TypeError, lambda: ops.boundary_confusion(t, t, 3, [1], tcm=torch.zeros(1, 4, 4, dtype=torch.int64)))):
        with pytest.raises(exc):
            call()


# ------------------------------------------------------------------------------------------------------------------ widths
def test_parse_boundary_widths():
    from cutmix_semisup_seg_amd.evaluation import parse_boundary_widths as parse, boundary_width_px as px
    got = parse('3,5,0.02')
    assert got == [3, 5, 0.02] and [type(v) for v in got] == [int, int, float]
    assert parse('1') == [1] and parse(' 254 , 0.5 ') == [254, 0.5] and parse('1,2,3,4') == [1, 2, 3, 4]
    for bad in ('', ',', '3,', '0', '255', '-1', '1,2,3,4,5', '1.0', '0.0', '3.5', 'wide', '1e2', 'nan', 'inf', '0.02;3', None, 3,
                [3, 5]):
        with pytest.raises(ValueError):
            parse(bad)
    # a ratio is of the image's own diagonal, rounded as Python rounds, at least 1
    assert px(7, (10, 10)) == 7
    assert px(0.02, (321, 321)) == int(round(0.02 * np.sqrt(2 * 321 * 321))) == 9
    assert px(0.02, (1024, 2048)) == 46 and px(0.02, (512, 1024)) == 23
    assert px(0.02, (5, 5)) == 1 and px(0.5, (3, 4)) == 2                   # round(2.5) == 2: Python's
    assert px(0.9, (400, 400)) == 254                                       # the widest band there is


def test_evaluator_constructor_refuses():
    from cutmix_semisup_seg_amd.evaluation import EvaluatorBoundary
    ev = EvaluatorBoundary(21, '3,0.02')
    assert ev.widths_spec == [3, 0.02] and ev.num_classes == 21
    for c, spec in ((21, []), (21, [1, 2, 3, 4, 5]), (21, [0]), (21, [255]), (21, [1.5]), (21, 'x'), (0, [1]), (65, [1])):
        with pytest.raises(ValueError):
            EvaluatorBoundary(c, spec)


def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_eval_seg_refuses_a_bad_spec_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import eval_seg
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    assert any(p.name == 'boundary_width' and p.default is None for p in eval_seg.experiment.params)
    for spec in ('', '0', '3,255', '1,2,3,4,5', 'wide', '1.5'):
        # no model file, no data set: the spec is looked at first
        res = CliRunner().invoke(eval_seg.experiment, [str(tmp_path / 'missing.pth'), '--dataset', 'pascal', '--boundary_width', spec])
        assert res.exit_code != 0 and not isinstance(res.exception, AssertionError), (res.output, res.exception)
        assert '--boundary_width' in res.output and 'does not load' not in res.output, res.output
    from cutmix_semisup_seg_amd.eval_seg import EvalNotRun, prepare
    with pytest.raises(EvalNotRun, match='boundary_width'):
        prepare(str(tmp_path / 'missing.pth'), 'pascal', 'val', '1', False, -1, 131, None, False, boundary_width='3,,5')
    # a good spec gets as far as the next refusal
    res = CliRunner().invoke(eval_seg.experiment, [str(tmp_path / 'missing.pth'), '--dataset', 'pascal', '--boundary_width', '3,0.02'])
    assert res.exit_code != 0 and 'does not load' in res.output


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_band_is_the_thresholded_distance_map():
    inp, ref = R.case('c5_void')
    t, c = inp['truth'], inp['c']
    for d in (1, 2, 5, 12, 254):
        for i in range(t.shape[0]):
            assert np.array_equal(R.band_map(t[i], c, d), (ref['dist_truth'][i] >= 1) & (ref['dist_truth'][i] <= d))
    assert (ref['dist_truth'][t == 255] == 0).all() and (ref['dist_truth'][t != 255] >= 1).all()
    assert (ref['dist_truth'][:, 0][t[:, 0] != 255] == 1).all()             # the array's edge
    inp, ref = R.case('checkerboard')
    assert (ref['dist_truth'] == 1).all() and (ref['dist_pred'] == 1).all()
    inp, ref = R.case('constant')
    yy, xx = np.mgrid[0:33, 0:41]
    assert np.array_equal(ref['dist_truth'][0], np.minimum(np.minimum(yy, 32 - yy), np.minimum(xx, 40 - xx)) + 1)


def test_reference_padding_cancels():
    inp, ref = R.case('c5_void')
    t, p, c, w = inp['truth'], inp['pred'], inp['c'], inp['widths']
    big_t = np.full((2, 33 + 11, 41 + 16), 255, dtype=np.uint8)
    big_p = np.zeros_like(big_t)
    big_t[:, 5:38, 7:48] = t
    big_p[:, 5:38, 7:48] = p
    bcm, tcm = R.confusion(big_t, big_p, c, w)
    assert np.array_equal(bcm, ref['bcm']) and np.array_equal(tcm, ref['tcm'])


# ------------------------------------------------------------------------------------------------------------------ host driver
def _request(truth, pred, classes, widths, **over):
    """-> (header, blocks)"""
    n, h, w = truth.shape
    head = dict(n=n, h=h, w=w, c=classes, ignore=255, k=widths.shape[1], maps=1)
    head.update(over)
    header = struct.pack('<7i', head['n'], head['h'], head['w'], head['c'], head['ignore'], head['k'], head['maps'])
    return header, [(widths, np.int32), (truth, np.uint8), (pred, np.uint8)]


def _result(raw, shape, c, k):
    return _hostcheck.split(raw, [('dist_truth', np.uint8, shape), ('dist_pred', np.uint8, shape), ('bcm', np.int64, (k, c + 1, c + 1)),
                                  ('tcm', np.int64, (k, c, c))])


@pytest.fixture(scope='module')
def hostcheck():
    exe = _hostcheck.build('hostcheck_boundary')

    def run(inp, program=exe, expect_code=0, **over):
        raw = _hostcheck.run(program, *_request(inp['truth'], inp['pred'], inp['c'], inp['widths'], **over), expect_code=expect_code)
        return None if raw is None else _result(raw, inp['truth'].shape, inp['c'], inp['widths'].shape[1])
    return run


def _same(got, ref):
    for key in ('dist_truth', 'dist_pred', 'bcm', 'tcm'):
        assert np.array_equal(got[key], ref[key]), key


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_vs_reference_every_pixel(hostcheck, name):
    inp, ref = R.case(name)
    _same(hostcheck(inp), ref)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_without_the_maps_the_walk_stops_at_the_widest_band(hostcheck, name):
    """what cms_boundary_confusion does when no distance output is asked for: the same matrices from maps capped per sample"""
    inp, ref = R.case(name)
    got = hostcheck(inp, maps=0)
    assert np.array_equal(got['bcm'], ref['bcm']) and np.array_equal(got['tcm'], ref['tcm'])
    cap = (inp['widths'].max(axis=1) + 1)[:, None, None]
    assert np.array_equal(got['dist_truth'], np.minimum(ref['dist_truth'], cap))
    assert np.array_equal(got['dist_pred'], np.minimum(ref['dist_pred'], cap))


def test_header_on_the_host_without_an_ignore_index(hostcheck):
    """ignore_index -1: no pixel is void, and 255 is a value like any other (no class: its pixels are not counted)"""
    inp, _ = R.case('c5_void')
    got = hostcheck(inp, ignore=-1)
    t = inp['truth']
    # a pixel whose truth is no class is counted nowhere, as cms_confusion counts it nowhere
    assert got['bcm'].sum() == inp['widths'].shape[1] * int((t != 255).sum())
    # truth 255 is a region of its own now: the distance map has no zero, and that of the prediction ignores the truth
    assert (got['dist_truth'] >= 1).all()
    assert np.array_equal(got['dist_pred'], R.dist_maps(np.zeros_like(t), inp['pred'], inp['c'])[1])


def test_header_on_the_host_64_classes(hostcheck):
    """C = 64: one width per counting launch (its two histograms take 33284 of the 65536 bytes)"""
    truth = (R.blobs((1, 40, 50), 64, 11, sigma=1.0)).astype(np.uint8)
    pred = (R.blobs((1, 40, 50), 64, 12, sigma=1.0)).astype(np.uint8)
    assert len(np.unique(truth)) > 20 and len(np.unique(pred)) > 20
    inp = dict(truth=truth, pred=pred, c=64, widths=np.array([[1, 3, 2]], dtype=np.int32))
    got = hostcheck(inp)
    bcm, tcm = R.confusion(truth, pred, 64, inp['widths'])
    assert np.array_equal(got['bcm'], bcm) and np.array_equal(got['tcm'], tcm)


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    inp, _ = R.case('c2_k1')
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(h=0), dict(w=-1), dict(k=0), dict(k=5), dict(h=2 ** 16, w=2 ** 15)):
        hostcheck(inp, expect_code=2, **over)


def test_stand_alone_under_the_host_sanitizers(hostcheck):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_boundary', sanitize=True)
    for name in ('one_pixel', 'row_of_7', 'c5_void', 'c21_void', 'wide', 'tall', 'long_row'):
        inp, ref = R.case(name)
        _same(hostcheck(inp, program=exe), ref)
