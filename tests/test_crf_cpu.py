"""
CPU-only: CRF refinement without a GPU.

  * the two new ABI symbols: declared, exported, prototyped, version 101; the descriptor's layout in C; the workspace sizes;
    every CMS_EINVAL case (decided before any HIP call)
  * ops.crf_refine's refusals, crf.CRFParams' parsing, eval_seg's `--crf*` refusals (the GPU never initialised)
  * the margins of the cases the host-check and GPU tests share (tests/_crf_refs.py), and the 2 % condition
  * the properties of the fp64 restatement itself
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
import _hostcheck
import _pascal_tree
import _crf_refs as R


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bsize_t\s+cms_crf_workspace_bytes\s*\(int n, int c, int H, int W\);', header)
    assert re.search(r'\bint\s+cms_crf_refine\s*\(const cms_crf_desc\* d, void\* workspace, size_t workspace_bytes, void\* stream\);',
                     header)
    for name in ('cms_crf_workspace_bytes', 'cms_crf_refine'):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_crf_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert _lib.PROTOTYPES['cms_crf_refine'] == (ctypes.c_int, [ctypes.POINTER(_lib.CrfDesc), ctypes.c_void_p, ctypes.c_size_t,
                                                                ctypes.c_void_p])
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    fields = [name for name, _ in _lib.CrfDesc._fields_]
    assert fields == ['logits', 'h', 'w', 'flip', 'n', 'c', 'H', 'W', 'k', 'align_corners', 'rgb', 'rect', 'radius', 'dilation',
                      'iters', 'bi_w', 'bi_xy', 'bi_rgb', 'pos_w', 'pos_xy', 'labels', 'label_dtype', 'ignore_index', 'cm',
                      'pred_out', 'q_out', 'stats']
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu", sizeof(cms_crf_desc));\n'
            + ''.join('printf(" %zu", offsetof(cms_crf_desc, {}));\n'.format(f) for f in fields) + 'return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.CrfDesc
    assert sizes == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


def test_workspace_bytes():
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_crf_workspace_bytes']
    up = lambda v: (v + 255) // 256 * 256
    # log P and two Q of (n, c, H, W) floats and one byte per pixel, each rounded up to 256
    for n, c, H, W in ((1, 1, 1, 1), (2, 21, 37, 53), (10, 21, 321, 321), (4, 19, 512, 1024), (1, 64, 5, 7)):
        assert f(n, c, H, W) == 3 * up(4 * n * c * H * W) + up(n * H * W), (n, c, H, W)
    for bad in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 65, 4, 4), (1, 3, 0, 4), (1, 3, 4, -1), (2, 3, 2 ** 15, 2 ** 15), (2 ** 31 - 1,) * 4):
        assert f(*bad) == 0, bad


def _desc(**over):
    """a descriptor cms_crf_refine would accept (host pointers: never dereferenced before the launch), then `over`
    -> (descriptor, workspace pointer, workspace bytes)"""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    rect = (ctypes.c_int32 * 8)(*over.pop('rect', (1, 1, 4, 5, 0, 0, 6, 7)))
    d = _lib.CrfDesc()
    d.logits[0], d.h[0], d.w[0] = p, 2, 3
    d.rgb, d.pred_out, d.stats, d.rect = p, p, p, ctypes.addressof(rect)
    d.n, d.c, d.H, d.W, d.k, d.align_corners = 2, 3, 6, 7, 1, 1
    d.radius, d.dilation, d.iters = 5, 3, 5
    d.bi_w, d.bi_xy, d.bi_rgb, d.pos_w, d.pos_xy = 4.0, 15.0, 13.0, 3.0, 3.0
    d._keep = (buf, rect)
    ws, ws_bytes = over.pop('workspace', p), over.pop('workspace_bytes', 2 ** 40)
    for key, val in over.items():
        if key in ('logits', 'h', 'w'):
            getattr(d, key)[0] = val
        else:
            setattr(d, key, val)
    return d, ws, ws_bytes


INF, NAN = float('inf'), float('nan')
BAD = [
    ('logits NULL', dict(logits=None)), ('rgb NULL', dict(rgb=None)), ('rect NULL', dict(rect_ptr=None)),
    ('stats NULL', dict(stats=None)), ('workspace NULL', dict(workspace=None)),
    ('views', dict(k=0)), ('views', dict(k=17)), ('num_classes', dict(c=0)), ('num_classes', dict(c=65)),
    ('geometry', dict(n=0)), ('geometry', dict(H=0)), ('geometry', dict(W=-1)), ('geometry', dict(h=0)), ('geometry', dict(w=-2)),
    ('radius', dict(radius=0)), ('radius', dict(radius=6)), ('dilation', dict(dilation=0)), ('dilation', dict(dilation=17)),
    ('iters', dict(iters=0)), ('iters', dict(iters=33)),
    ('weights', dict(bi_w=-1.0)), ('weights', dict(pos_w=-0.5)), ('weights', dict(bi_w=INF)), ('weights', dict(pos_w=NAN)),
    ('theta', dict(bi_xy=0.0)), ('theta', dict(bi_rgb=-1.0)), ('theta', dict(pos_xy=NAN)), ('theta', dict(bi_rgb=INF)),
    ('cm given without labels', dict(cm_self=True)), ('nothing to produce', dict(pred_out=None)),
    ('label dtype', dict(labels_self=True, label_dtype=7)),
    ('2^31', dict(n=2, H=2 ** 15, W=2 ** 15)), ('2^31', dict(n=1, H=2 ** 31 - 1, W=2 ** 31 - 1)),
    ('rectangle', dict(rect=(-1, 1, 4, 5, 0, 0, 6, 7))), ('rectangle', dict(rect=(1, -1, 4, 5, 0, 0, 6, 7))),
    ('rectangle', dict(rect=(1, 1, 0, 5, 0, 0, 6, 7))), ('rectangle', dict(rect=(1, 1, 4, 0, 0, 0, 6, 7))),
    ('leaves the canvas', dict(rect=(1, 1, 6, 5, 0, 0, 6, 7))), ('leaves the canvas', dict(rect=(1, 1, 4, 7, 0, 0, 6, 7))),
    ('leaves the canvas', dict(rect=(1, 1, 4, 5, 0, 0, 7, 7))), ('leaves the canvas', dict(rect=(6, 0, 1, 1, 0, 0, 6, 7))),
    ('leaves the canvas', dict(rect=(1, 1, 2 ** 31 - 1, 5, 0, 0, 6, 7))),
    ('workspace too small', dict(workspace_bytes=0)),
]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_crf_refine']
    err = _lib.fn['cms_last_error']
    assert f(None, None, 0, None) == -1 and b'NULL descriptor' in err()
    for what, over in BAD:
        over = dict(over)
        special = {k: over.pop(k) for k in ('rect_ptr', 'cm_self', 'labels_self') if k in over}
        d, ws, ws_bytes = _desc(**over)
        if 'rect_ptr' in special:
            d.rect = None
        if 'cm_self' in special:
            d.cm = d.rgb
        if 'labels_self' in special:
            d.labels = d.rgb
        assert f(ctypes.byref(d), ws, ws_bytes, None) == -1, (what, over)
        msg = err().decode()
        assert all(w in msg for w in what.split()), (what, over, msg)
    need = _lib.fn['cms_crf_workspace_bytes'](2, 3, 6, 7)
    d, ws, _ = _desc()
    assert f(ctypes.byref(d), ws, need - 1, None) == -1 and b'too small' in err()
    assert f(ctypes.byref(d), ws + 8, 2 ** 40, None) == -1 and b'misaligned' in err()
    d.stats = d.stats + 4
    assert f(ctypes.byref(d), ws, 2 ** 40, None) == -1 and b'stats misaligned' in err()


# ------------------------------------------------------------------------------------------------------------------ the op
def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_op_refusals(monkeypatch):
    import torch
    from cutmix_semisup_seg_amd import ops
    from cutmix_semisup_seg_amd.crf import CRFParams
    _no_gpu(monkeypatch)
    lg = torch.zeros(2, 3, 4, 5)
    rgb = torch.zeros(2, 3, 8, 9, dtype=torch.uint8)
    rects = np.array([[0, 0, 8, 9], [1, 2, 3, 4]], dtype=np.int32)
    prm = CRFParams()
    ok = dict(logits_list=[lg], flips=[False], rgb=rgb, rects=rects, num_classes=3, out_size=(8, 9), params=prm)

    def refused(exc, what, **over):
        with pytest.raises(exc, match=what):
            ops.crf_refine(**dict(ok, **over))
    refused(RuntimeError, 'GPU only')                                                  # CPU tensors, everything else in order
    refused(TypeError, 'float32', logits_list=[lg.double()])
    refused(TypeError, r'\(N,C,h,w\)', logits_list=[lg[0]])
    refused(ValueError, 'views', logits_list=[])
    refused(ValueError, 'views', logits_list=[lg] * 17, flips=[False] * 17)
    refused(ValueError, 'flips', flips=[False, True])
    refused(ValueError, 'num_classes', num_classes=65)
    refused(ValueError, 'a view of shape', num_classes=4)
    refused(TypeError, 'uint8', rgb=rgb.float())
    refused(ValueError, 'rgb of shape', rgb=rgb[:, :, :7])
    refused(TypeError, 'rects', rects=rects.astype(np.float32))
    refused(TypeError, 'rects', rects=rects[:1])
    refused(ValueError, 'rectangle', rects=np.array([[0, 0, 9, 9], [1, 2, 3, 4]]))
    refused(ValueError, 'rectangle', rects=np.array([[0, 0, 8, 9], [1, 2, 0, 4]]))
    refused(ValueError, 'rectangle', rects=np.array([[0, -1, 8, 9], [1, 2, 3, 4]]))
    refused(TypeError, 'labels', labels=torch.zeros(2, 8, 9))
    refused(ValueError, 'labels of shape', labels=torch.zeros(2, 8, 8, dtype=torch.uint8))
    refused(ValueError, 'cm given without labels', cm=torch.zeros(3, 3, dtype=torch.int64))
    refused(TypeError, 'cm must be', labels=torch.zeros(2, 8, 9, dtype=torch.uint8), cm=torch.zeros(3, 3))
    refused(TypeError, 'pred must be', pred=torch.zeros(2, 8, 9))
    refused(TypeError, 'stats_out', stats_out=torch.zeros(2))
    refused(ValueError, '2\\^31', out_size=(2 ** 15, 2 ** 15), rgb=rgb)
    refused(TypeError, 'params lacks', params=dict(radius=1))
    for key, val in (('radius', 0), ('radius', 6), ('dilation', 17), ('iters', 0), ('iters', 33), ('bi_w', -1.0), ('pos_w', INF),
                     ('bi_xy', 0.0), ('bi_rgb', NAN), ('pos_xy', -2.0), ('radius', 2.5)):
        refused(ValueError, key, params=dict(prm.as_dict(), **{key: val}))


def test_crf_params_parsing():
    from cutmix_semisup_seg_amd.crf import CRFParams, DEFAULTS
    assert DEFAULTS == dict(iters=5, radius=5, dilation=3, bi_w=4.0, bi_xy=15.0, bi_rgb=13.0, pos_w=3.0, pos_xy=3.0)
    assert CRFParams().as_dict() == DEFAULTS
    p = CRFParams(iters='7', radius=2, dilation=' 16 ', bi_w='0', bi_xy='2.5', bi_rgb=1e-3, pos_w=0, pos_xy='1e2')
    assert p.as_dict() == dict(iters=7, radius=2, dilation=16, bi_w=0.0, bi_xy=2.5, bi_rgb=1e-3, pos_w=0.0, pos_xy=100.0)
    assert isinstance(p.iters, int) and isinstance(p.bi_w, float)
    assert CRFParams(iters=None, radius=1).as_dict() == dict(DEFAULTS, radius=1)
    for key, bad in (('iters', 0), ('iters', 33), ('iters', '2.5'), ('iters', 'many'), ('iters', 2.5), ('iters', True), ('iters', ''),
                     ('radius', 0), ('radius', 6), ('radius', '-1'), ('dilation', 0), ('dilation', 17), ('dilation', 'x'),
                     ('bi_w', -1), ('bi_w', 'nan'), ('bi_w', 'inf'), ('bi_w', 'heavy'), ('bi_w', 1e39), ('pos_w', '-0.1'),
                     ('bi_xy', 0), ('bi_xy', '-3'), ('bi_rgb', 'nan'), ('bi_rgb', ''), ('pos_xy', 0.0), ('pos_xy', 'inf')):
        with pytest.raises(ValueError, match=key):
            CRFParams(**{key: bad})
    with pytest.raises(ValueError, match='unknown'):
        CRFParams(sigma=3)
    assert CRFParams.from_options(False) is None and CRFParams.from_options(False, crf_iters=None) is None
    assert CRFParams.from_options(True, crf_iters='3', crf_bi_w=None).as_dict() == dict(DEFAULTS, iters=3)
    with pytest.raises(ValueError, match='--crf_radius is given without --crf'):
        CRFParams.from_options(False, crf_radius='2')


@pytest.fixture(scope='module')
def small_model(tmp_path_factory):
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    path = tmp_path_factory.mktemp('crf_model')
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    checkpoint.save_model(net, str(path / 'model.pth'))
    return str(path / 'model.pth')


def test_eval_seg_crf_refusals_come_before_the_model_and_the_gpu(tmp_path, monkeypatch, small_model):
    from click.testing import CliRunner
    import eval_seg
    from cutmix_semisup_seg_amd import checkpoint
    _no_gpu(monkeypatch)
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), {'a': (20, 24), 'b': (22, 20), 'c': (20, 20)}, ['a', 'b'], ['c'])
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    opened = []
    load = checkpoint.load_model
    monkeypatch.setattr(checkpoint, 'load_model', lambda path: opened.append(path) or load(path))
    ok = [small_model, '--dataset', 'pascal']

    def refused(args, what):
        res = CliRunner().invoke(eval_seg.experiment, ok + args)
        assert res.exit_code != 0, res.output
        assert not isinstance(res.exception, AssertionError), res.exception
        assert what in res.output, (args, res.output)
        assert not opened                                                             # said before the model file is opened
    for opt, bad in (('iters', '0'), ('iters', '33'), ('iters', 'x'), ('iters', '2.5'), ('radius', '6'), ('radius', '0'),
                     ('dilation', '17'), ('dilation', '-1'), ('bi_w', '-1'), ('bi_w', 'nan'), ('bi_xy', '0'), ('bi_rgb', 'inf'),
                     ('pos_w', 'much'), ('pos_xy', '-3')):
        refused(['--crf', '--crf_' + opt, bad], opt)
    for opt in ('iters', 'radius', 'dilation', 'bi_w', 'bi_xy', 'bi_rgb', 'pos_w', 'pos_xy'):
        refused(['--crf_' + opt, '3'], '--crf_{} is given without --crf'.format(opt))
    # with everything in order the program gets as far as the GPU, and only there is it stopped
    res = CliRunner().invoke(eval_seg.experiment, ok + ['--crf', '--crf_iters', '2'])
    assert isinstance(res.exception, AssertionError) and 'the GPU was touched' in str(res.exception) and opened


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_case_margins(name):
    """The conditions on the INPUTS of the host-check and GPU tests: no near-tie at any pixel, and a refinement that does something."""
    inp, ref = R.case(name)
    print(name, 'min top-two gap of Q^T', ref['gap'], '4 B', 4 * R.B, 'unary gap', ref['unary_gap'], 'changed', ref['changed'])
    assert ref['gap'] >= 4 * R.B
    assert ref['unary_gap'] >= R.T.gap_bound(inp['k'])
    assert ref['changed'] >= R.MIN_CHANGED
    assert max(np.abs(l).max() for l in inp['logits']) <= 8.0
    assert len(inp['logits']) == inp['k'] and (inp['k'] == 1 or any(inp['flips']))
    assert ref['stats'][0] == sum(int(r[2]) * int(r[3]) for r in inp['rects'])
    assert ref['cm'].sum() == (inp['labels'] != 255).sum()


def test_cases_cover_what_they_should():
    specs = list(R.CASES.values())
    assert {s['c'] for s in specs} >= {2, 5, 21, 64}
    assert {(s['radius'], s['dilation']) for s in specs} >= {(1, 1), (2, 3), (5, 3), (5, 16)}
    assert {s['iters'] for s in specs} == {1, 5} and {s['k'] for s in specs} == {1, 3} and {s['align'] for s in specs} == {True, False}
    main = R.CASES['c21_r5s3_t5_k1']
    assert main['shape'] == (2, 37, 53) and main['rects'][0] != main['rects'][1]
    assert all(37 - r[2] == 3 and 53 - r[3] == 4 for r in main['rects'])
    assert 5 * 16 > 53                                                                # the last window is larger than the image
    assert R.CASES['tiny_5x7']['shape'] == (1, 5, 7)
    assert any(tuple(r[2:]) == (1, 1) for r in R.CASES['one_pixel']['rects'])
    assert all(tuple(r) == (0, 0, 37, 53) for r in R.CASES['full_canvas']['rects'])


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _refine(inp, **over):
    a = dict(inp, **over)
    return R.refine(a['logits'], a['flips'], a['rgb'], a['rects'], a['size'], a['align'], a['radius'], a['dilation'], a['iters'],
                    **a['prm'])


def test_reference_sample_alone_equals_the_sample_in_its_batch_at_another_offset():
    inp, ref = R.case('c5_r2s3_t5_k3')
    top, left, h, w = inp['rects'][1]
    # sample 1 alone, its rectangle moved to the canvas' corner: P and the image are moved with it
    p, _, _ = R.unary(inp['logits'], inp['flips'], inp['size'], inp['align'])
    p1 = np.zeros((1,) + p.shape[1:])
    p1[0, :, :h, :w] = p[1, :, top:top + h, left:left + w]
    p1[0, :, h:, :] = 1.0 / p.shape[1]
    p1[0, :, :, w:] = 1.0 / p.shape[1]
    rgb1 = np.zeros((1,) + inp['rgb'].shape[1:], dtype=np.uint8)
    rgb1[0, :, :h, :w] = inp['rgb'][1, :, top:top + h, left:left + w]
    q1 = R.mean_field(p1, rgb1, [(0, 0, h, w)], inp['radius'], inp['dilation'], inp['iters'], **inp['prm'])
    assert np.array_equal(q1[0, :, :h, :w], ref['q'][1, :, top:top + h, left:left + w])


def test_reference_without_weights_is_the_unary_prediction():
    inp, ref = R.case('c21_r5s3_t5_k1')
    got = _refine(inp, prm=dict(inp['prm'], bi_w=0.0, pos_w=0.0))
    p, upred, _ = R.unary(inp['logits'], inp['flips'], inp['size'], inp['align'])
    assert np.array_equal(got['pred'], upred) and got['stats'][1] == 0
    assert np.abs(got['q'] - p).max() <= 1e-14                                        # softmax(log P) = P


def test_reference_constant_image_makes_the_bilateral_kernel_a_second_spatial_one():
    inp, _ = R.case('c5_r2s3_t5_k3')
    grey = np.full_like(inp['rgb'], 97)
    prm = inp['prm']
    got = _refine(inp, rgb=grey)
    # w_b exp(-d2 / (2 a^2)) + w_g exp(-d2 / (2 g^2)): with a = g the two add up to one spatial kernel of weight w_b + w_g
    one = _refine(inp, rgb=grey, prm=dict(prm, bi_xy=prm['pos_xy']))
    two = _refine(inp, rgb=grey, prm=dict(prm, bi_w=0.0, pos_w=prm['bi_w'] + prm['pos_w']))
    assert np.abs(one['q'] - two['q']).max() <= 1e-13
    # ... and the colour bandwidth no longer matters
    assert np.array_equal(got['q'], _refine(inp, rgb=grey, prm=dict(prm, bi_rgb=1.0))['q'])
    assert not np.array_equal(got['q'], R.case('c5_r2s3_t5_k3')[1]['q'])


def test_reference_neighbour_count_and_one_pixel():
    _, count = R.pair_weights(np.zeros((3, 5, 7)), 2, 3, 1.0, 1.0, 1.0, 1.0, 1.0)
    assert count[0, 0] == 2 * 3 - 1 and count[2, 3] == 1 * 3 - 1 and count[4, 6] == 2 * 3 - 1          # steps of 3 in a 5 x 7 image
    _, count = R.pair_weights(np.zeros((3, 1, 1)), 5, 1, 1.0, 1.0, 1.0, 1.0, 1.0)
    assert count.tolist() == [[0]]
    inp, ref = R.case('one_pixel')
    p, upred, _ = R.unary(inp['logits'], inp['flips'], inp['size'], inp['align'])
    assert ref['pred'][0, 2, 3] == upred[0, 2, 3] and np.abs(ref['q'][0, :, 2, 3] - p[0, :, 2, 3]).max() <= 1e-14
