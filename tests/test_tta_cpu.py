"""
CPU-only: test-time augmentation without a GPU.

  * the two new ABI symbols: declared, exported, prototyped; every CMS_EINVAL case (decided before any HIP call)
  * tta.TTA / parse_scales: the view-size table, the view order, every refusal
  * the fp64 restatement of the vote and the resize (tests/_tta_refs.py) against itself and against a second formulation, and the
    margins of the cases the GPU test shares
  * eval_seg's refusals through click's runner, the GPU never initialised
  * csrc/tta_math.hpp -- the functions the kernels of csrc/tta.hip are made of -- driven on the host by a small program of its
    own (tests/hostcheck_tta) over every pixel of the GPU test's cases and over block-edge sizes, against the fp64
    restatement; and the same stand-alone program once more under the host's address and undefined-behaviour sanitizers
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
import _pascal_tree
import _tta_refs as R



# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+cms_tta_resize\s*\(const void\* src, void\* dst, int n, int c, int H, int W, int Hs, int Ws, int dtype, '
                     r'int flip,\s*void\* stream\);', header)
    assert re.search(r'\bint\s+cms_tta_vote\s*\(const cms_tta_desc\* d, void\* stream\);', header)
    assert '#define CMS_TTA_MAX_VIEWS 16' in header
    for name in ('cms_tta_resize', 'cms_tta_vote'):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_tta_vote'] == (ctypes.c_int, [ctypes.POINTER(_lib.TtaDesc), ctypes.c_void_p])
    assert _lib.PROTOTYPES['cms_tta_resize'] == (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 8 + [ctypes.c_void_p])


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
            'sizeof(cms_tta_desc), offsetof(cms_tta_desc, h), offsetof(cms_tta_desc, flip), offsetof(cms_tta_desc, n), '
            'offsetof(cms_tta_desc, labels), offsetof(cms_tta_desc, pred_out)); return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.TtaDesc
    assert sizes == [ctypes.sizeof(D), D.h.offset, D.flip.offset, D.n.offset, D.labels.offset, D.pred_out.offset]


def _desc(**over):
    """a descriptor cms_tta_vote would accept (host pointers: never dereferenced before the launch), then `over`"""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    d = _lib.TtaDesc()
    d.n, d.c, d.H, d.W, d.k, d.align_corners = 1, 3, 4, 4, 2, 1
    for i in range(2):
        d.logits[i], d.h[i], d.w[i], d.flip[i] = p, 2, 2, i
    d.labels, d.label_dtype, d.ignore_index, d.cm, d.pred_out = p, 0, 255, p, p
    d._keep = buf
    for key, val in over.items():
        if isinstance(val, tuple):
            getattr(d, key)[val[0]] = val[1]
        else:
            setattr(d, key, val)
    return d


BAD_VOTES = [
    ('k', dict(k=0)), ('k', dict(k=-1)), ('k', dict(k=17)),
    ('num_classes', dict(c=0)), ('num_classes', dict(c=65)), ('num_classes', dict(c=-3)),
    ('geometry', dict(n=0)), ('geometry', dict(H=0)), ('geometry', dict(W=-1)),
    ('geometry', dict(h=(1, 0))), ('geometry', dict(w=(0, -2))),
    ('NULL', dict(logits=(1, None))), ('NULL', dict(logits=(0, None))),
    ('without labels', dict(labels=None)),
    ('nothing to produce', dict(cm=None, pred_out=None)), ('nothing to produce', dict(cm=None, pred_out=None, labels=None)),
    ('label dtype', dict(label_dtype=7)),
    ('2^31', dict(n=2, H=2 ** 15, W=2 ** 15)), ('2^31', dict(n=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)),
]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_tta_vote']
    assert f(None, None) == -1 and b'NULL descriptor' in _lib.fn['cms_last_error']()
    for what, over in BAD_VOTES:
        d = _desc(**over)
        assert f(ctypes.byref(d), None) == -1, over
        assert what.encode() in _lib.fn['cms_last_error'](), (over, _lib.fn['cms_last_error']())
    with pytest.raises(ValueError, match='tta_vote'):
        _lib.check(f(ctypes.byref(_desc(k=0)), None), 'cms_tta_vote')


def test_bad_resize_arguments_return_einval_before_any_hip_call():
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_tta_resize']
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    #       src dst n  c  H  W  Hs Ws dtype flip
    good = (p, p, 1, 3, 4, 4, 2, 2, 0, 0)
    bad = [good[:i] + (None,) + good[i + 1:] for i in (0, 1)]
    bad += [good[:i] + (v,) + good[i + 1:] for i in range(2, 8) for v in (0, -1)]
    bad += [good[:8] + (2,) + good[9:], good[:8] + (-1,) + good[9:]]
    bad.append((p, p, 2, 1, 2 ** 15, 2 ** 15, 2, 2, 0, 0))
    bad.append((p, p, 2, 1, 2, 2, 2 ** 15, 2 ** 15, 0, 0))
    bad.append((p, p) + (2 ** 31 - 1,) * 6 + (0, 0))
    for args in bad:
        assert f(*args, None) == -1, args
        assert b'tta_resize' in _lib.fn['cms_last_error']()


def test_ops_check_their_arguments_before_the_library():
    import torch
    from cutmix_semisup_seg_amd import ops
    lg = [torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 4, 4)]
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.tta_vote(lg, [False, True], 3, (4, 4), want_pred=True)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.tta_resize(torch.zeros(1, 3, 4, 4), (2, 2))
    for exc, call in (
            (ValueError, lambda: ops.tta_vote([], [], 3, (4, 4), want_pred=True)),
            (ValueError, lambda: ops.tta_vote(lg * 9, [False] * 18, 3, (4, 4), want_pred=True)),
            (ValueError, lambda: ops.tta_vote(lg, [False], 3, (4, 4), want_pred=True)),
            (ValueError, lambda: ops.tta_vote(lg, [False, True], 4, (4, 4), want_pred=True)),
            (ValueError, lambda: ops.tta_vote(lg, [False, True], 3, (0, 4), want_pred=True)),
            (ValueError, lambda: ops.tta_vote(lg, [False, True], 3, (4, 4))),
            (ValueError, lambda: ops.tta_vote(lg, [False, True], 3, (4, 4), cm=torch.zeros(3, 3, dtype=torch.int64))),
            (ValueError, lambda: ops.tta_vote([lg[0], torch.zeros(2, 3, 2, 2)], [False, True], 3, (4, 4), want_pred=True)),
            (ValueError, lambda: ops.tta_vote(lg, [False, True], 3, (4, 4), labels=torch.zeros(1, 5, 4, dtype=torch.uint8))),
            (TypeError, lambda: ops.tta_vote(lg, [False, True], 3, (4, 4), labels=torch.zeros(1, 4, 4))),
            (TypeError, lambda: ops.tta_vote(lg, [False, True], 3, 4, want_pred=True)),
            (TypeError, lambda: ops.tta_vote([lg[0][0]], [False], 3, (4, 4), want_pred=True)),
            (TypeError, lambda: ops.tta_vote(lg, [False, True], 3, (4, 4), labels=torch.zeros(1, 4, 4, dtype=torch.uint8),
                                             cm=torch.zeros(3, 3))),
            (TypeError, lambda: ops.tta_resize(torch.zeros(1, 3, 4, 4, dtype=torch.float64), (2, 2))),
            (TypeError, lambda: ops.tta_resize(torch.zeros(3, 4, 4), (2, 2))),
            (ValueError, lambda: ops.tta_resize(torch.zeros(1, 3, 4, 4), (0, 2))),
            (TypeError, lambda: ops.tta_resize(torch.zeros(1, 3, 4, 4), 2))):
        with pytest.raises(exc):
            call()


# ------------------------------------------------------------------------------------------------------------------ view geometry
def test_view_size_table():
    from cutmix_semisup_seg_amd.tta import TTA
    t = TTA((0.5, 0.75, 1, 1.25), False)
    assert t.view_size((41, 57), (1, 1), 0.5) == (21, 29)
    assert t.view_size((64, 96), (32, 32), 0.75) == (64, 64)
    assert t.view_size((64, 96), (32, 32), 0.1) == (32, 32)
    for canvas, block in (((41, 57), (1, 1)), ((64, 96), (32, 32)), ((321, 321), (1, 1))):
        assert t.view_size(canvas, block, 1) == canvas
    assert t.view_size((41, 57), (1, 1), 1.25) == (51, 71)                   # 51.25, 71.25
    assert t.view_size((64, 96), (32, 32), 1.25) == (96, 128)                # 2.5 -> 3 blocks, 3.75 -> 4
    assert t.view_size((321, 321), (1, 1), 0.75) == (241, 241)               # 240.75
    assert t.view_size((64, 96), (32, 32)) == [(32, 64), (64, 64), (64, 96), (96, 128)]
    for s in (0.3, 0.5, 0.75, 1.0, 1.5, 1.75):                               # the definition, at sizes of all parities
        for hc in range(1, 70):
            for b in (1, 8, 32):
                got = TTA((s,)).view_size((hc * b, hc * b), (b, b), s)[0]
                assert got == b * max(1, int(np.floor(s * hc + 0.5))) and got % b == 0 and got >= b


def test_view_order_and_limits():
    from cutmix_semisup_seg_amd.tta import TTA, parse_scales
    assert parse_scales('0.5,0.75,1') == (0.5, 0.75, 1.0) and parse_scales(' 1.5 , 1 ') == (1.5, 1.0)
    assert TTA().views() == [(1.0, False)]
    assert TTA((1.25, 0.5), False).views() == [(1.25, False), (0.5, False)]
    assert TTA((1.25, 0.5), True).views() == [(1.25, False), (1.25, True), (0.5, False), (0.5, True)]
    assert len(TTA(tuple(0.25 * i for i in range(1, 9)), True).views()) == 16
    assert len(TTA(tuple(0.25 * i for i in range(1, 17)), False).views()) == 16


@pytest.mark.parametrize('text', ['', ' ', ',', '1,', '1,,2', 'big', '1;2', '0.5,x', '0', '-1', '1,0', '1,-0.5', 'nan', 'inf', '1,1',
                                  '0.5,1,0.50'])
def test_parse_scales_refusals(text):
    from cutmix_semisup_seg_amd.tta import parse_scales
    with pytest.raises(ValueError, match='scales'):
        parse_scales(text)


def test_tta_refusals():
    from cutmix_semisup_seg_amd.tta import TTA
    for scales in ((), (0.0,), (-1.0, 1.0), (1.0, 1.0), ('a',), (float('nan'),)):
        with pytest.raises(ValueError, match='scales'):
            TTA(scales, False)
    with pytest.raises(ValueError, match='at most 16'):
        TTA(tuple(0.25 * i for i in range(1, 10)), True)                     # 9 scales flipped: 18 views
    with pytest.raises(ValueError, match='at most 16'):
        TTA(tuple(0.25 * i for i in range(1, 18)), False)


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('align', [True, False])
def test_reference_upsample_vs_a_second_formulation_and_torch(align):
    import torch
    rng = np.random.RandomState(3)
    for (h, w), (H, W) in (((5, 7), (37, 53)), ((60, 80), (37, 53)), ((1, 1), (4, 3)), ((9, 13), (1, 1)), ((4, 6), (4, 6))):
        x = rng.standard_normal((2, 3, h, w))
        want = np.einsum('Yy,ncyx,Xx->ncYX', R.interp_matrix(H, h, align), x, R.interp_matrix(W, w, align))
        got = R.upsample(x, (H, W), align)
        assert np.abs(got - want).max() <= 1e-13
        t = torch.nn.functional.interpolate(torch.from_numpy(x), size=(H, W), mode='bilinear', align_corners=align).numpy()
        assert np.abs(got - t).max() <= 1e-12
        assert np.abs(R.upsample(x, (H, W), align, flip=True) - R.upsample(x[..., ::-1], (H, W), align)).max() == 0.0


def test_reference_resize_is_interpolate_without_antialiasing():
    import torch
    for shape, size, flip in R.RESIZE_CASES:
        x = R.resize_input(shape).astype(np.float64)
        t = torch.nn.functional.interpolate(torch.from_numpy(x), size=size, mode='bilinear', align_corners=False).numpy()
        assert np.abs(R.resize(x, size, flip) - (t[..., ::-1] if flip else t)).max() <= 1e-12
    x = R.resize_input((1, 2, 6, 5)).astype(np.float64)
    assert np.array_equal(R.resize(x, (6, 5)), x) and np.array_equal(R.resize(x, (6, 5), True), x[..., ::-1])


@pytest.mark.parametrize('align', [True, False])
def test_reference_one_view_is_the_argmax_of_the_upsample(align):
    lg, _ = R.make_views(1, 7, 2, seed=1)
    score, pred, _ = R.vote(lg, [False], (37, 53), align)
    up = np.einsum('Yy,ncyx,Xx->ncYX', R.interp_matrix(37, lg[0].shape[2], align), lg[0].astype(np.float64),
                   R.interp_matrix(53, lg[0].shape[3], align))
    assert np.abs(score - up).max() <= 1e-13 and np.array_equal(pred, up.argmax(axis=1))


def test_reference_mirrored_view_flipped_is_the_view_unflipped():
    lg, _ = R.make_views(3, 5, 2, seed=4)
    for k in (1, 3):
        a = R.vote(lg[:k], [False] * k, (37, 53), True)
        b = R.vote([l[..., ::-1] for l in lg[:k]], [True] * k, (37, 53), True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_reference_constant_view_changes_nothing():
    lg, flips = R.make_views(3, 6, 2, seed=5)
    a = R.vote(lg, flips, (37, 53), False)
    const = np.full((2, 6, 4, 4), 2.5, dtype=np.float32)                      # softmax = 1 / C for every class
    b = R.vote(lg + [const], flips + [True], (37, 53), False)
    assert np.array_equal(a[1], b[1]) and np.abs((b[0] - a[0]) - 1.0 / 6).max() <= 1e-15


@pytest.mark.parametrize('k,c', sorted(R.VOTE_CASES))
def test_vote_case_margins(k, c):
    """The condition on the INPUTS of tests/test_gpu_tta.py's vote cases: no near-tie at any pixel."""
    case = R.vote_case(k, c)
    print('k', k, 'C', c, 'min top-two gap', case['gap'].min(), 'bound', R.gap_bound(k))
    assert case['gap'].min() >= R.gap_bound(k)
    assert max(np.abs(l).max() for l in case['logits']) <= 8.0
    sizes = {l.shape[2:] for l in case['logits']}
    assert len(sizes) == min(k, 4) and any(case['flips']) and not all(case['flips'])
    assert all(w % 2 == 1 or (h, w) == (60, 80) for h, w in sizes)
    assert len(np.unique(case['pred'])) > 1 and (case['labels'] == 255).any()
    assert case['cm'].sum() == (case['labels'] != 255).sum()


# ------------------------------------------------------------------------------------------------------------------ eval_seg
def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


@pytest.fixture(scope='module')
def small_model(tmp_path_factory):
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    path = tmp_path_factory.mktemp('tta_model')
    out = {}
    for c in (21, 2):
        net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], c, np.zeros(3), np.ones(3))
        out[c] = str(path / 'model{}.pth'.format(c))
        checkpoint.save_model(net, out[c])
    return out


def test_eval_seg_refusals_come_before_the_gpu(tmp_path, monkeypatch, small_model):
    from click.testing import CliRunner
    import eval_seg
    _no_gpu(monkeypatch)
    sizes = {'a': (20, 24), 'b': (22, 20), 'c': (20, 20)}
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), sizes, ['a', 'b'], ['c'])
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'garbage.pth').write_bytes(b'not a pickle at all')
    import torch
    torch.save({'weights': torch.zeros(3)}, str(tmp_path / 'dict.pth'))
    ok = [small_model[21], '--dataset', 'pascal']

    def refused(args, what, env=None):
        res = CliRunner().invoke(eval_seg.experiment, args, env=env)
        assert res.exit_code != 0, res.output
        assert not isinstance(res.exception, AssertionError), res.exception          # ... and not because the GPU was reached
        assert what in res.output, (args, res.output)

    refused([str(tmp_path / 'missing.pth'), '--dataset', 'pascal'], 'does not load')
    refused([str(tmp_path / 'garbage.pth'), '--dataset', 'pascal'], 'does not load')
    refused([str(tmp_path / 'dict.pth'), '--dataset', 'pascal'], 'not a whole network')
    refused(ok + ['--subset', 'test'], 'leaves no test set')
    refused(ok + ['--bin_fill_holes'], 'binary')
    refused([small_model[2], '--dataset', 'pascal'], 'predicts 2 classes')
    for scales in ('', '0', '1,1', 'wide', '1,-2'):
        refused(ok + ['--scales', scales], 'scales')
    refused(ok + ['--scales', '0.25,0.5,0.75,1,1.25,1.5,1.75,2,2.25', '--flip'], 'at most 16')
    refused(ok, 'one GPU', env={'WORLD_SIZE': '2'})
    refused([small_model[21], '--dataset', 'camvid'], 'camvid')                       # no `camvid` key in [paths]
    (tmp_path / 'semantic_segmentation.cfg').write_text('[paths]\nisic2017=/nowhere.zip\n')
    refused(ok, 'pascal_voc')                                                        # the key this data set needs is missing
    # with everything in order the program gets as far as the GPU, and only there is it stopped
    _pascal_tree.write_config(str(tmp_path), root)
    res = CliRunner().invoke(eval_seg.experiment, ok + ['--scales', '0.75,1', '--flip'])
    assert isinstance(res.exception, AssertionError) and 'the GPU was touched' in str(res.exception)


# ------------------------------------------------------------------------------------------------------------------ host driver
def _vote_request(logits, flips, size, align, n=None, c=None, k=None):
    """-> (header, blocks) of a vote request"""
    n = logits[0].shape[0] if n is None else n
    c = logits[0].shape[1] if c is None else c
    header = struct.pack('<7i', 0, n, c, size[0], size[1], len(logits) if k is None else k, int(align))
    for l, fl in zip(logits, flips):
        header += struct.pack('<3i', l.shape[2], l.shape[3], int(fl))
    return header, [(l, np.float32) for l in logits]


def _resize_request(x, size, flip):
    return struct.pack('<8i', 1, *x.shape, size[0], size[1], int(flip)), [(x, np.float32)]


@pytest.fixture(scope='module')
def hostcheck():
    exe = _hostcheck.build('hostcheck_tta')

    def run(request, shape, dtype, program=exe, expect_code=0):
        raw = _hostcheck.run(program, *request, expect_code=expect_code)
        return None if raw is None else _hostcheck.split(raw, [('out', dtype, shape)])['out']
    return run


@pytest.mark.parametrize('k,c', sorted(R.VOTE_CASES))
def test_header_on_the_host_vs_reference_every_pixel(hostcheck, k, c):
    case = R.vote_case(k, c)
    n, H, W = R.OUT
    got = hostcheck(_vote_request(case['logits'], case['flips'], (H, W), case['align']), (n, H, W), np.uint8)
    assert np.array_equal(got, case['pred'])


# output sizes at which the launch takes another shape: one pixel, one short of / exactly / one past a block of 256, several blocks
# with a grid-stride tail; one view (resampled, identity, identity flipped) and several
EDGES = [(1, 1, 1, 1, 3), (1, 1, 1, 2, 3), (1, 3, 85, 1, 4), (1, 16, 16, 1, 4), (1, 1, 257, 2, 2), (2, 16, 16, 3, 5), (3, 31, 29, 2, 7),
         (1, 255, 1, 4, 3)]


@pytest.mark.parametrize('n,H,W,k,c', EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize('align', [True, False])
def test_header_on_the_host_block_edges(hostcheck, n, H, W, k, c, align):
    for seed in range(3):
        logits, flips = R.make_views(k, c, n, seed, sizes=[(3, 5), (H, W), (7, 3), (2 * H + 1, W + 2)])
        if k == 1:
            flips = [seed == 2]
        _, pred, gap = R.vote(logits, flips, (H, W), align)
        got = hostcheck(_vote_request(logits, flips, (H, W), align), (n, H, W), np.uint8)
        sure = gap >= (R.gap_bound(k) if k > 1 else 1e-4)                 # one view: logits of magnitude 8 interpolated in fp32
        assert sure.mean() >= 0.95 and np.array_equal(got[sure], pred[sure])
        assert got.max() < c


@pytest.mark.parametrize('shape,size,flip', R.RESIZE_CASES + [((1, 1, 4, 300), (3, 257), True), ((1, 2, 7, 5), (1, 1), False)])
def test_header_on_the_host_resize(hostcheck, shape, size, flip):
    x = R.resize_input(shape)
    got = hostcheck(_resize_request(x, size, flip), shape[:2] + tuple(size), np.float32)
    np.testing.assert_allclose(got, R.resize(x, size, flip), rtol=1e-5, atol=1e-6)
    if flip:
        plain = hostcheck(_resize_request(x, size, False), shape[:2] + tuple(size), np.float32)
        assert np.array_equal(got, plain[..., ::-1])


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    logits, flips = R.make_views(2, 3, 1, 0)
    for over in (dict(k=0), dict(k=17), dict(c=0), dict(c=65), dict(n=0)):
        hostcheck(_vote_request(logits, flips, (4, 4), True, **over), None, None, expect_code=2)
    hostcheck(_vote_request(logits, flips, (0, 4), True), None, None, expect_code=2)
    hostcheck(_vote_request(logits, flips, (2 ** 16, 2 ** 15), True), None, None, expect_code=2)
    hostcheck(_resize_request(R.resize_input((1, 1, 2, 2)), (0, 3), False), None, None, expect_code=2)


def test_stand_alone_under_the_host_sanitizers(hostcheck):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_tta', sanitize=True)
    n, H, W = R.OUT
    for k, c in ((16, 64), (5, 19), (2, 2)):
        case = R.vote_case(k, c)
        got = hostcheck(_vote_request(case['logits'], case['flips'], (H, W), case['align']), (n, H, W), np.uint8, program=exe)
        assert np.array_equal(got, case['pred'])
    for flip in (False, True):                                                 # one view: resampled, and identity mirrored
        logits, _ = R.make_views(1, 5, 2, 7, sizes=[(5, 7)])
        hostcheck(_vote_request(logits, [flip], (37, 53), True), (2, 37, 53), np.uint8, program=exe)
        got = hostcheck(_vote_request(logits, [flip], (5, 7), False), (2, 5, 7), np.uint8, program=exe)
        want = logits[0].argmax(axis=1)
        assert np.array_equal(got, want[..., ::-1] if flip else want)
    for shape, size, flip in R.RESIZE_CASES:
        x = R.resize_input(shape)
        got = hostcheck(_resize_request(x, size, flip), shape[:2] + tuple(size), np.float32, program=exe)
        np.testing.assert_allclose(got, R.resize(x, size, flip), rtol=1e-5, atol=1e-6)
