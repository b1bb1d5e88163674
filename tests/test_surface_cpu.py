"""
CPU-only: the surface distances (HD, HD95, ASSD) without a GPU.

  * the two new ABI symbols: declared, exported, prototyped, version 101; the descriptor's layout in C; the workspace sizes;
    every CMS_EINVAL case (decided before any HIP call), with its message
  * ops.surface_distances' refusals; EvaluatorSurface's constructor; eval_seg taking --surface_dist and still refusing a missing model
    first, the GPU never touched
  * the reference itself (tests/_surface_refs.py): the conditions on its cases that keep the GPU tests from passing emptily; padding
    cancels, a translated image gives the same numbers, equal maps give zeros, HD95 <= HD, ASSD <= HD
  * csrc/surface_math.hpp -- the functions the kernels of csrc/surface.hip are made of -- driven on the host by a small program of
    its own (tests/hostcheck_surface) over every pixel of the GPU test's cases, against the scipy reference; and the same
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
import _surface_refs as R



# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bsize_t\s+cms_surface_workspace_bytes\s*\(int n, int h, int w, int num_classes\);', header)
    assert re.search(r'\bint\s+cms_surface_distances\s*\(const cms_surface_desc\* d, void\* stream\);', header)
    for name in ('cms_surface_workspace_bytes', 'cms_surface_distances'):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_surface_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert _lib.PROTOTYPES['cms_surface_distances'] == (ctypes.c_int, [ctypes.POINTER(_lib.SurfaceDesc), ctypes.c_void_p])
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    fields = [name for name, _ in _lib.SurfaceDesc._fields_]
    assert fields == ['truth', 'pred', 'n', 'h', 'w', 'num_classes', 'ignore_index', 'stats', 'sums', 'd2_pred', 'd2_truth',
                      'workspace', 'workspace_bytes']
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu", sizeof(cms_surface_desc));\n'
            + ''.join('printf(" %zu", offsetof(cms_surface_desc, {}));\n'.format(f) for f in fields) + 'return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.SurfaceDesc
    assert sizes == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


def _a16(b):
    return (b + 15) // 16 * 16


def _workspace(n, h, w, c):
    """the layout csrc/surface_math.hpp documents, restated: counts and select histograms, select state, partial sums per slab of
    4096 pixels (at most 64 slabs), the two surface maps, the two d2 maps, the row distances of both maps per class"""
    pix, nc = n * h * w, n * c
    slabs = min(64, max(1, -(-h * w // 4096)))
    return (_a16(nc * 8) + _a16(nc * 2048) + _a16(nc * 32) + _a16(nc * slabs * 32) + 2 * _a16(pix) + 2 * _a16(4 * pix)
            + 2 * _a16(2 * pix * c))


def test_workspace_bytes():
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_surface_workspace_bytes']
    assert f(1, 1, 1, 2) == 16 + 4096 + 64 + 64 + 2 * 16 + 2 * 16 + 2 * 16 == 4336
    assert f(3, 33, 41, 5) == 153600
    for shape in ((1, 1, 1, 1), (3, 33, 41, 5), (3, 67, 130, 21), (10, 321, 321, 21), (4, 512, 1024, 19), (1, 1024, 2048, 19),
                  (1, 16384, 16384, 64), (70000, 1, 1, 64), (2, 40, 50, 64)):
        assert f(*shape) == _workspace(*shape), shape
    for bad in ((0, 4, 4, 2), (1, 0, 4, 2), (1, 4, -1, 2), (-2, 4, 4, 2), (1, 4, 4, 0), (1, 4, 4, 65), (1, 4, 4, -1),
                (1, 16385, 4, 2), (1, 4, 16385, 2), (8, 16384, 16384, 2), (2 ** 31 - 1, 1, 1, 2), (2 ** 31 - 1,) * 3 + (2,)):
        assert f(*bad) == 0, bad
    assert f(7, 16384, 16384, 1) > 0                                        # 7 * 2^28 pixels: below 2^31
    # a workgroup of the reduction per (sample, class, slab): their number stays below 2^31 as well
    assert f(2 ** 25, 1, 1, 63) > 0 and f(2 ** 25, 1, 1, 64) == 0


def _desc(**over):
    """a descriptor cms_surface_distances would accept (host pointers: never dereferenced before the launch), then `over`"""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    d = _lib.SurfaceDesc()
    d.truth, d.pred, d.stats, d.sums, d.d2_pred, d.d2_truth, d.workspace = (p,) * 7
    d.n, d.h, d.w, d.num_classes, d.ignore_index = 1, 4, 4, 3, 255
    d.workspace_bytes = 2 ** 50
    d._keep = buf
    for key, val in over.items():
        setattr(d, key, val)
    return d


BAD = [
    ('truth NULL', dict(truth=None)), ('pred NULL', dict(pred=None)), ('workspace NULL', dict(workspace=None)),
    ('nothing to produce', dict(stats=None, sums=None, d2_pred=None, d2_truth=None)),
    ('num_classes', dict(num_classes=0)), ('num_classes', dict(num_classes=65)), ('num_classes', dict(num_classes=-3)),
    ('geometry', dict(n=0)), ('geometry', dict(n=-1)), ('geometry', dict(h=0)), ('geometry', dict(w=-2)),
    ('16384', dict(h=16385)), ('16384', dict(w=16385)), ('16384', dict(w=2 ** 31 - 1)),
    ('2^31', dict(n=8, h=16384, w=16384)), ('2^31', dict(n=2 ** 31 - 1, h=2, w=2)),
    ('2^31', dict(n=2 ** 25, h=1, w=1, num_classes=64)),
    ('workspace too small', dict(workspace_bytes=_workspace(1, 4, 4, 3) - 1)), ('workspace too small', dict(workspace_bytes=0)),
]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_surface_distances']
    assert f(None, None) == -1 and b'NULL descriptor' in _lib.fn['cms_last_error']()
    for what, over in BAD:
        d = _desc(**over)
        assert f(ctypes.byref(d), None) == -1, over
        assert what.encode() in _lib.fn['cms_last_error'](), (over, _lib.fn['cms_last_error']())
        assert _lib.fn['cms_last_error']().startswith(b'surface_distances: ')
    d = _desc()
    d.workspace = d.workspace + 8
    assert f(ctypes.byref(d), None) == -1 and b'aligned' in _lib.fn['cms_last_error']()
    with pytest.raises(ValueError, match='surface'):
        _lib.check(f(ctypes.byref(_desc(num_classes=99)), None), 'cms_surface_distances')
    # (that stats, sums and the d2 outputs may be NULL in the combinations left is tests/test_gpu_surface.py's to show: an accepted
    # descriptor launches)


def test_ops_check_their_arguments_before_the_library():
    import torch
    from cutmix_semisup_seg_amd import ops
    t = torch.zeros(2, 8, 9, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.surface_distances(t, t, 3)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.surface_distances(t[0], t[0], 3, ignore_index=None, want_maps=True)
    for exc, call in (
            (TypeError, lambda: ops.surface_distances(t.long(), t, 3)),
            (TypeError, lambda: ops.surface_distances(t, t.float(), 3)),
            (TypeError, lambda: ops.surface_distances(t.numpy(), t, 3)),
            (ValueError, lambda: ops.surface_distances(t, t[:, :, :8], 3)),
            (ValueError, lambda: ops.surface_distances(t, t[0], 3)),
            (ValueError, lambda: ops.surface_distances(t[None], t[None], 3)),
            (ValueError, lambda: ops.surface_distances(t[:0], t[:0], 3)),
            (ValueError, lambda: ops.surface_distances(t, t, 0)),
            (ValueError, lambda: ops.surface_distances(t, t, 65)),
            (ValueError, lambda: ops.surface_distances(torch.zeros(1, 1, 16385, dtype=torch.uint8), torch.zeros(1, 1, 16385, dtype=torch.uint8), 2))):
        with pytest.raises(exc):
            call()


def test_evaluator_constructor_refuses():
    from cutmix_semisup_seg_amd.evaluation import EvaluatorSurface
    ev = EvaluatorSurface(21)
    assert ev.num_classes == 21
    for c in (0, 65, -1):
        with pytest.raises(ValueError):
            EvaluatorSurface(c)
    # nothing sampled: nothing scored, and no device needed to say so
    assert np.isnan(ev.hd95()).all() and np.isnan(ev.hd()).all() and np.isnan(ev.assd()).all()
    assert [a.tolist() for a in ev.pairs()] == [[0] * 21, [0] * 21] and np.isnan(EvaluatorSurface.headline(ev.hd()))


def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_eval_seg_takes_the_flag_and_still_refuses_a_missing_model_first(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import eval_seg
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    assert any(p.name == 'surface_dist' and p.is_flag and p.default is False for p in eval_seg.experiment.params)
    res = CliRunner().invoke(eval_seg.experiment, [str(tmp_path / 'missing.pth'), '--dataset', 'pascal', '--surface_dist'])
    assert res.exit_code != 0 and not isinstance(res.exception, AssertionError), (res.output, res.exception)
    assert 'does not load' in res.output and 'no such option' not in res.output.lower()
    res = CliRunner().invoke(eval_seg.experiment, [str(tmp_path / 'missing.pth'), '--dataset', 'pascal', '--surface_dist', '--crf',
                                                   '--boundary_width', '3'])
    assert res.exit_code != 0 and 'does not load' in res.output


# ------------------------------------------------------------------------------------------------------------------ the reference
def _n(stats):
    return stats[..., 0] + stats[..., 1]


def test_reference_cases_reach_what_they_are_there_for():
    """so that no GPU test passes emptily"""
    refs = {name: R.case(name)[1] for name in R.CASES}
    for name, ref in refs.items():
        sc = R.scored(ref['stats'])
        print(name, 'scored', int(sc.sum()), 'one-sided', int(R.one_sided(ref['stats']).sum()), 'max d2', int(ref['stats'][..., 2:4].max()))
    st = refs['one_pixel']['stats']
    assert R.scored(st).sum() == 0 and R.one_sided(st).sum() == 2
    st = refs['one_pixel_hit']['stats']
    assert st[0, 0].tolist() == [1, 1, 0, 0, 0, 0] and st[0, 1].tolist() == [0, 0, -1, -1, -1, -1]
    assert R.scored(refs['c5_void']['stats']).sum() >= 8 and R.scored(refs['c21_void']['stats']).sum() >= 30
    assert not R.scored(refs['c21_void']['stats'])[2].any() and (refs['c21_void']['stats'][2, :, :2] == 0).all()     # all void
    assert R.one_sided(refs['one_sided']['stats']).sum() >= 2 and R.scored(refs['one_sided']['stats']).sum() >= 6
    assert (refs['one_sided']['stats'][:, 3, 0] == 0).all() and refs['one_sided']['stats'][1, 4, 1] == 0
    assert refs['very_tall']['stats'][..., 2:4].max() == 4199 ** 2 > 2 ** 24
    assert refs['very_wide']['stats'][..., 2:4].max() == 4199 ** 2
    assert refs['tall']['stats'][..., 2:4].max() > 65535
    assert (refs['same']['stats'][..., 2:][R.scored(refs['same']['stats'])] == 0).all() and (refs['same']['sums'] == 0).all()
    assert R.scored(refs['same']['stats']).sum() >= 8
    assert (refs['checkerboard']['d2_pred'] == 1).all() and (refs['checkerboard']['d2_truth'] == 1).all()
    assert _n(refs['n21']['stats'])[0, 1] == 21 and _n(refs['n2']['stats'])[0, 1] == 2
    # far_corner: the corners, the tie at 5 and the decoy one row further off than the same-row pixel
    st = refs['far_corner']['stats']
    assert st[0, 1].tolist() == [1, 1] + [66 ** 2 + 129 ** 2] * 4
    assert st[0, 2, 2] == 25 and st[0, 3, 2] == 25 and st[0, 3, 3] == 36
    every = [ref['stats'][R.scored(ref['stats'])] for ref in refs.values()]
    assert any((((_n(s) - 1) % 20) == 0).any() for s in every) and any((s[:, 4] != s[:, 5]).any() for s in every)
    assert R.scored(refs['c64']['stats']).sum() >= 64


def test_reference_padding_and_translation_cancel():
    inp, ref = R.case('c5_void')
    t, p, c = inp['truth'], inp['pred'], inp['c']
    for top, left, bottom, right in ((5, 7, 6, 9), (0, 3, 11, 0)):
        big_t = np.full((2, 33 + top + bottom, 41 + left + right), 255, dtype=np.uint8)
        big_p = R.blobs(big_t.shape, c, 77)
        big_t[:, top:top + 33, left:left + 41] = t
        big_p[:, top:top + 33, left:left + 41] = p
        got = R.reference(big_t, big_p, c)
        assert np.array_equal(got['stats'], ref['stats']) and np.array_equal(got['sums'], ref['sums'])
        assert np.array_equal(got['d2_pred'][:, top:top + 33, left:left + 41], ref['d2_pred'])
        assert (got['d2_pred'] >= 0).sum() == (ref['d2_pred'] >= 0).sum()


def test_reference_orderings():
    for name in ('c2', 'c5_void', 'c21_void', 'tall', 'far_corner', 'c64'):
        ref = R.case(name)[1]
        sc = R.scored(ref['stats'])
        assert (ref['hd95'][sc] <= ref['hd'][sc]).all() and (ref['assd'][sc] <= ref['hd'][sc]).all()
        assert np.isnan(ref['hd'][~sc]).all() and not np.isnan(ref['hd'][sc]).any()
        # the integer ranks are numpy.percentile's
        st = ref['stats'][sc]
        r = (19 * (_n(st) - 1)) % 20
        hd95 = np.sqrt(st[:, 4]) + r / 20.0 * (np.sqrt(st[:, 5]) - np.sqrt(st[:, 4]))
        assert np.allclose(hd95, ref['hd95'][sc], rtol=1e-12, atol=0)
    ref = R.case('same')[1]
    assert (ref['hd'][R.scored(ref['stats'])] == 0).all()


def test_reference_lines():
    ds = R.dataset([R.case('one_sided')[1], R.case('c5_void')[1]])
    out = R.lines('VAL', ds)
    assert len(out) == 7 and out[0].startswith('VAL HD95=') and out[2].startswith('VAL ASSD=') and out[4].startswith('VAL HD=')
    assert out[6] == '-- surface pairs 4, 4, 4, 2, 3 (one-sided 0, 0, 0, 2, 1)'
    ds = R.dataset([R.case('one_pixel')[1]])
    assert R.lines('TEST', ds) == ['TEST HD95=nan', '-- HD95 -, -', 'TEST ASSD=nan', '-- ASSD -, -', 'TEST HD=nan', '-- HD -, -',
                                   '-- surface pairs 0, 0 (one-sided 1, 1)']


# ------------------------------------------------------------------------------------------------------------------ host driver
def _request(truth, pred, classes, **over):
    """-> (header, blocks)"""
    n, h, w = truth.shape
    head = dict(n=n, h=h, w=w, c=classes, ignore=255)
    head.update(over)
    return struct.pack('<5i', head['n'], head['h'], head['w'], head['c'], head['ignore']), [(truth, np.uint8), (pred, np.uint8)]


def _result(raw, shape, c):
    return _hostcheck.split(raw, [('stats', np.int64, (shape[0], c, 6)), ('sums', np.float64, (shape[0], c, 2)),
                                  ('d2_pred', np.int32, shape), ('d2_truth', np.int32, shape)])


@pytest.fixture(scope='module')
def hostcheck():
    exe = _hostcheck.build('hostcheck_surface')

    def run(inp, program=exe, expect_code=0, **over):
        raw = _hostcheck.run(program, *_request(inp['truth'], inp['pred'], inp['c'], **over), expect_code=expect_code)
        return None if raw is None else _result(raw, inp['truth'].shape, inp['c'])
    return run


def _same(got, ref):
    for key in ('stats', 'd2_pred', 'd2_truth'):
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key
    assert R.sums_close(got['sums'], ref['sums'], ref['stats'])


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_vs_reference_every_pixel(hostcheck, name):
    inp, ref = R.case(name)
    _same(hostcheck(inp), ref)


def test_header_on_the_host_without_an_ignore_index(hostcheck):
    """ignore_index -1: no pixel is void, and 255 is a value like any other (no class: on nobody's surface, outside every mask)"""
    inp, _ = R.case('c5_void')
    _same(hostcheck(inp, ignore=-1), R.reference(inp['truth'], inp['pred'], inp['c'], ignore=None))


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    inp, _ = R.case('c2')
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(h=0), dict(w=-1), dict(h=16385), dict(n=8, h=16384, w=16384)):
        hostcheck(inp, expect_code=2, **over)


def test_stand_alone_under_the_host_sanitizers(hostcheck):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_surface', sanitize=True)
    for name in R.SMALL:
        inp, ref = R.case(name)
        _same(hostcheck(inp, program=exe), ref)
