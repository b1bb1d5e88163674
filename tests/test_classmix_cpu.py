"""
CPU-only: ClassMix without a GPU.

  * the two new ABI symbols: declared, exported, prototyped, version 101; the descriptor's layout in C; the workspace sizes;
    every CMS_EINVAL case (decided before any HIP call)
  * ops.classmix_mask's refusals; mask_gen.ClassMixGenerator's draw order
  * the command line of train_seg_semisup_classmix_mt: the CutMix trainer's minus the five --boxmask_* options and --mask_prop_range;
    its refusals, which come before the GPU
  * the margins of the cases the GPU test shares (tests/_classmix_refs.py)
  * csrc/classmix_math.hpp -- the functions the kernels of csrc/classmix.hip are made of -- driven on the host by a small program of
    its own (tests/hostcheck_classmix) over every pixel of the GPU test's cases and over sizes at which the walk takes
    another shape, against the fp64 restatement; and the same stand-alone program once more under the host's address and
    undefined-behaviour sanitizers
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
import _classmix_refs as R



# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bsize_t\s+cms_classmix_workspace_bytes\s*\(int n, int H, int W\);', header)
    assert re.search(r'\bint\s+cms_classmix\s*\(const cms_classmix_desc\* d, void\* stream\);', header)
    for name in ('cms_classmix_workspace_bytes', 'cms_classmix'):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_classmix_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _lib.PROTOTYPES['cms_classmix'] == (ctypes.c_int, [ctypes.POINTER(_lib.ClassMixDesc), ctypes.c_void_p])
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    fields = [name for name, _ in _lib.ClassMixDesc._fields_]
    assert fields == ['logits', 'valid', 'keys', 'n', 'c', 'h', 'w', 'H', 'W', 'align_corners', 'mask_out', 'pred_out', 'present_out',
                      'chosen_out', 'workspace', 'workspace_bytes']
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu", sizeof(cms_classmix_desc));\n'
            + ''.join('printf(" %zu", offsetof(cms_classmix_desc, {}));\n'.format(f) for f in fields) + 'return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.ClassMixDesc
    assert sizes == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


def test_workspace_bytes():
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_classmix_workspace_bytes']
    # 256 slot words of 8 bytes per sample, then one byte per pixel rounded up to 16
    assert f(1, 1, 1) == 2048 + 16
    assert f(3, 33, 41) == 3 * 2048 + 4064                                  # 4059 pixels
    assert f(10, 321, 321) == 10 * 2048 + 1030416                           # 1030410
    assert f(4, 512, 1024) == 4 * 2048 + 4 * 512 * 1024
    assert f(65535, 1, 1) == 65535 * 2048 + 65536
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (-2, 4, 4), (2, 2 ** 15, 2 ** 15), (65536, 1, 1), (2 ** 31 - 1,) * 3):
        assert f(*bad) == 0, bad
    assert f(1, 2 ** 15, 2 ** 16 - 1) > 0 and f(1, 2 ** 15, 2 ** 16) == 0     # 2^31 - 2^15 pixels, 2^31 pixels


def _desc(**over):
    """a descriptor cms_classmix would accept (host pointers: never dereferenced before the launch), then `over`"""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    d = _lib.ClassMixDesc()
    d.logits, d.valid, d.keys, d.mask_out, d.pred_out, d.present_out, d.chosen_out, d.workspace = (p,) * 8
    d.n, d.c, d.h, d.w, d.H, d.W, d.align_corners = 1, 3, 2, 2, 4, 4, 1
    d.workspace_bytes = 2 ** 40
    d._keep = buf
    for key, val in over.items():
        setattr(d, key, val)
    return d


BAD = [
    ('NULL', dict(logits=None)), ('NULL', dict(keys=None)), ('NULL', dict(mask_out=None)), ('NULL', dict(workspace=None)),
    ('num_classes', dict(c=0)), ('num_classes', dict(c=65)), ('num_classes', dict(c=-3)),
    ('geometry', dict(n=0)), ('geometry', dict(n=-1)), ('geometry', dict(h=0)), ('geometry', dict(w=-2)), ('geometry', dict(H=0)),
    ('geometry', dict(W=-1)),
    ('65535', dict(n=65536, H=1, W=1)),
    ('2^31', dict(n=2, H=2 ** 15, W=2 ** 15)), ('2^31', dict(n=1, H=2 ** 31 - 1, W=2 ** 31 - 1)),
    ('2^31', dict(c=64, h=2 ** 13, w=2 ** 13)),
    ('workspace', dict(workspace_bytes=2048 + 16 - 1)), ('workspace', dict(workspace_bytes=0)),
]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_classmix']
    assert f(None, None) == -1 and b'NULL descriptor' in _lib.fn['cms_last_error']()
    for what, over in BAD:
        d = _desc(**over)
        assert f(ctypes.byref(d), None) == -1, over
        assert what.encode() in _lib.fn['cms_last_error'](), (over, _lib.fn['cms_last_error']())
    d = _desc()
    d.workspace = d.workspace + 8
    assert f(ctypes.byref(d), None) == -1 and b'aligned' in _lib.fn['cms_last_error']()
    with pytest.raises(ValueError, match='classmix'):
        _lib.check(f(ctypes.byref(_desc(c=0)), None), 'cms_classmix')
    # (that valid, pred_out, present_out and chosen_out may be NULL is tests/test_gpu_classmix.py's to show: an accepted descriptor
    # launches)


def test_ops_check_their_arguments_before_the_library():
    import torch
    from cutmix_semisup_seg_amd import ops
    lg = torch.zeros(2, 3, 4, 4)
    keys = np.zeros((2, 3))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.classmix_mask(lg, keys, (8, 8))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.classmix_mask(lg, torch.zeros(2, 3, dtype=torch.float64), (8, 8))
    nan = keys.copy()
    nan[1, 2] = np.nan
    inf = keys.copy()
    inf[0, 0] = np.inf
    for exc, call in (
            (ValueError, lambda: ops.classmix_mask(lg, np.zeros((2, 4)), (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, np.zeros((3, 3)), (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, np.zeros((6,)), (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, torch.zeros(2, 2, dtype=torch.float64), (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, nan, (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, inf, (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, torch.from_numpy(nan), (8, 8))),
            (ValueError, lambda: ops.classmix_mask(lg, keys, (0, 8))),
            (ValueError, lambda: ops.classmix_mask(torch.zeros(2, 65, 4, 4), np.zeros((2, 65)), (8, 8))),
            (TypeError, lambda: ops.classmix_mask(lg, keys, 8)),
            (TypeError, lambda: ops.classmix_mask(lg[0], keys, (8, 8)))):
        with pytest.raises(exc):
            call()


# ------------------------------------------------------------------------------------------------------------------ generator
def test_generate_params_draw_order():
    from cutmix_semisup_seg_amd import mask_gen
    g = mask_gen.ClassMixGenerator()
    assert g.needs_teacher and not hasattr(g, 'generate_ranges')
    keys = g.generate_params(5, 21, rng=np.random.RandomState(42))
    want = np.random.RandomState(42).random_sample((5, 21))
    assert keys.dtype == np.float64 and keys.shape == (5, 21) and np.array_equal(keys, want)
    assert keys.min() >= 0.0 and keys.max() < 1.0
    # one call per batch and nothing else: the stream is where that one draw leaves it
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    g.generate_params(3, 4, rng=r1)
    r2.random_sample((3, 4))
    assert r1.uniform() == r2.uniform()


# ------------------------------------------------------------------------------------------------------------------ command
def _table(command):
    return [(p.name, type(p.type).__name__, p.default, getattr(p, 'is_flag', False)) for p in command.params]


def test_option_table_is_the_cutmix_trainers_minus_six():
    import train_seg_semisup_mask_mt as cutmix
    import train_seg_semisup_classmix_mt as cm
    base = _table(cutmix.experiment)
    gone = ['mask_prop_range', 'boxmask_n_boxes', 'boxmask_fixed_aspect_ratio', 'boxmask_by_size', 'boxmask_outside_bounds',
            'boxmask_no_invert']
    assert all(any(t[0] == g for t in base) for g in gone)
    want = [t for t in base if t[0] not in gone]
    got = _table(cm.experiment)
    assert [t[0] for t in got] == [t[0] for t in want] and len(got) == len(base) - 6
    assert got == want                                               # every shared option keeps its type and default
    mode = [p for p in cm.experiment.params if p.name == 'mask_mode'][0]
    assert list(mode.type.choices) == ['mix'] and mode.default == 'mix'
    assert cm.train_seg_semisup_classmix_mt is not None


def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_command_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_classmix_mt as cm
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    base = ['--synthetic', '--crop_size', '33,33']
    res = CliRunner().invoke(cm.experiment, base)                                       # no --freeze_bn
    assert res.exit_code != 0 and isinstance(res.exception, ValueError), (res.output, res.exception)
    assert '--freeze_bn' in str(res.exception)
    # the DeepLab v3+ head stays on batch statistics (and draws dropout noise) whatever --freeze_bn says
    res = CliRunner().invoke(cm.experiment, base + ['--freeze_bn', '--arch', 'resnet101_deeplabv3plus_imagenet'])
    assert res.exit_code != 0 and isinstance(res.exception, ValueError), (res.output, res.exception)
    assert '--freeze_bn' in str(res.exception) and 'BatchNorm' in str(res.exception)
    for extra in (['--mask_mode', 'zero'], ['--mask_prop_range', '0.5'], ['--boxmask_n_boxes', '2']):
        res = CliRunner().invoke(cm.experiment, base + ['--freeze_bn'] + extra)
        assert res.exit_code == 2 and not isinstance(res.exception, AssertionError), (res.output, res.exception)
    # with everything in order the program gets as far as the GPU, and only there is it stopped
    res = CliRunner().invoke(cm.experiment, base + ['--freeze_bn'])
    assert isinstance(res.exception, AssertionError) and 'the GPU was touched' in str(res.exception)


def test_prepass_check_leaves_the_network_as_it_found_it():
    from architectures import deeplab2
    from cutmix_semisup_seg_amd.train_seg_semisup_mask_mt import teacher_prepass_moves
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 3, np.zeros(3), np.ones(3))
    net.eval()
    net.layer1.train()
    before = [m.training for m in net.modules()]
    assert teacher_prepass_moves(net, True) is None
    why = teacher_prepass_moves(net, False)
    assert why and '--freeze_bn' in why
    assert [m.training for m in net.modules()] == before


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_case_margins(name):
    """The condition on the INPUTS of tests/test_gpu_classmix.py's cases: no near-tie at any pixel."""
    inp, ref = R.case(name)
    n, c = inp['logits'].shape[:2]
    print(name, 'min top-two gap', ref['gap'], 'present', [bin(p).count('1') for p in ref['present']])
    assert ref['gap'] >= R.MARGIN
    for p, ch in zip(ref['present'], ref['chosen']):
        assert ch & ~p == 0 and bin(ch).count('1') == (bin(p).count('1') + 1) // 2 and p < 2 ** c
    if name == 'c64':
        assert ref['present'][1] >> 63 == 1 and ref['chosen'][1] >> 63 == 1
    if name == 'slots':
        assert inp['size'][0] * inp['size'][1] > 4 * 1024 * 8                  # several slot words per sample
    if c > 2:
        assert all(0.0 < float(m.mean()) < 1.0 for m in ref['mask'])


def test_reference_properties():
    inp = R.case_inputs('main_ac')
    lg, keys, size = inp['logits'], inp['keys'], inp['size']
    ref = R.classmix(lg, keys, size, True)
    # equal keys are ordered by class index: the chosen half is the lowest present classes
    eq = R.classmix(lg, np.zeros_like(keys), size, True)
    for p, ch in zip(eq['present'], eq['chosen']):
        classes = [c for c in range(21) if p >> c & 1]
        assert ch == R.bits(classes[:(len(classes) + 1) // 2])
    # a class that occurs only where valid == 0 is not present; an all-invalid sample has nothing
    valid = np.ones((3,) + size, dtype=np.float32)
    cls = int(ref['pred'][0, 0, 0])
    valid[0][ref['pred'][0] == cls] = 0.0
    valid[2] = 0.0
    v = R.classmix(lg, keys, size, True, valid)
    assert v['present'][0] == ref['present'][0] & ~(1 << cls) and v['present'][1] == ref['present'][1] and v['present'][2] == 0
    assert v['chosen'][2] == 0 and float(v['mask'][2].max()) == 0.0 and float(v['mask'][0, 0][valid[0] == 0].max()) == 0.0
    # a sample alone is the sample in its batch
    one = R.classmix(lg[1:2], keys[1:2], size, True)
    assert np.array_equal(one['mask'][0], ref['mask'][1]) and one['chosen'][0] == ref['chosen'][1]


# ------------------------------------------------------------------------------------------------------------------ host driver
def _request(logits, keys, size, align, valid=None, **over):
    """-> (header, blocks)"""
    n, c, h, w = logits.shape
    head = dict(n=n, c=c, h=h, w=w, H=size[0], W=size[1])
    head.update(over)
    header = struct.pack('<8i', head['n'], head['c'], head['h'], head['w'], head['H'], head['W'], int(align), int(valid is not None))
    return header, [(keys, np.float64), (logits, np.float32)] + ([(valid, np.float32)] if valid is not None else [])


def _result(raw, n, size):
    out = _hostcheck.split(raw, [('pred', np.uint8, (n,) + tuple(size)), ('sets', np.uint64, (2, n)),
                                 ('mask', np.float32, (n, 1) + tuple(size))])
    sets = out['sets']
    return dict(pred=out['pred'], present=[int(v) for v in sets[0]], chosen=[int(v) for v in sets[1]], mask=out['mask'])


@pytest.fixture(scope='module')
def hostcheck():
    exe = _hostcheck.build('hostcheck_classmix')

    def run(logits, keys, size, align, valid=None, program=exe, expect_code=0, **over):
        raw = _hostcheck.run(program, *_request(logits, keys, size, align, valid, **over), expect_code=expect_code)
        return None if raw is None else _result(raw, logits.shape[0], size)
    return run


def _same(got, ref):
    assert np.array_equal(got['pred'], ref['pred'])
    assert got['present'] == ref['present'] and got['chosen'] == ref['chosen']
    assert np.array_equal(got['mask'], ref['mask'])


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_vs_reference_every_pixel(hostcheck, name):
    inp, ref = R.case(name)
    _same(hostcheck(inp['logits'], inp['keys'], inp['size'], inp['align']), ref)


def test_header_on_the_host_with_a_validity_map(hostcheck):
    inp, ref = R.case('main_ac')
    valid = np.ones((3,) + inp['size'], dtype=np.float32)
    valid[0][ref['pred'][0] == int(ref['pred'][0, 0, 0])] = 0.0
    valid[1, ::2, 1::3] = 0.0
    valid[1, 5, 5] = -2.5                                                 # any non-zero value is valid
    valid[2] = 0.0
    _same(hostcheck(inp['logits'], inp['keys'], inp['size'], inp['align'], valid),
          R.classmix(inp['logits'], inp['keys'], inp['size'], inp['align'], valid))


# output sizes at which the walk takes another shape: fewer than four pixels per sample (no 16-byte group), sample starts at every
# residue of four, one short of / exactly / one past a workgroup's 1024 pixels, an odd number of pixels in several samples
EDGES = [(1, 1, 1), (3, 1, 1), (5, 1, 3), (4, 1, 2), (3, 3, 3), (2, 1, 1023), (2, 32, 32), (3, 25, 41), (2, 5, 413)]


@pytest.mark.parametrize('n,H,W', EDGES, ids=lambda v: str(v))
def test_header_on_the_host_walk_edges(hostcheck, n, H, W):
    for seed, (c, align) in enumerate(((5, True), (3, False))):
        rng = np.random.RandomState(100 * seed + n + H + W)
        logits = rng.standard_normal((n, c, 3, 4)).astype(np.float32)
        keys = rng.random_sample((n, c))
        valid = (rng.uniform(size=(n, H, W)) < 0.8).astype(np.float32) if seed else None
        ref = R.classmix(logits, keys, (H, W), align, valid)
        got = hostcheck(logits, keys, (H, W), align, valid)
        # no seed search here: compare where the fp64 top-two gap leaves no doubt, which must be nearly everywhere
        up = R.T.upsample(logits, (H, W), align)
        top = np.sort(up, axis=1)
        sure = (top[:, -1] - top[:, -2]) >= 1e-4
        assert sure.mean() >= 0.95 and np.array_equal(got['pred'][sure], ref['pred'][sure])
        if sure.all():
            _same(got, ref)
        # whatever the predictions are, the sets and the mask follow from them
        for i in range(n):
            ok = np.ones((H, W), dtype=bool) if valid is None else valid[i] != 0
            assert got['present'][i] == R.bits(set(got['pred'][i][ok].tolist()))
            first = [cl for cl in range(c) if got['chosen'][i] >> cl & 1]
            assert np.array_equal(got['mask'][i, 0], (ok & np.isin(got['pred'][i], first)).astype(np.float32))


def test_host_driver_refuses_what_the_library_refuses(hostcheck):
    inp = R.case_inputs('c2')
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(h=0), dict(w=-1), dict(H=0), dict(W=0), dict(n=65536),
                 dict(H=2 ** 16, W=2 ** 15)):
        hostcheck(inp['logits'], inp['keys'], inp['size'], True, expect_code=2, **over)


def test_stand_alone_under_the_host_sanitizers(hostcheck):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_classmix', sanitize=True)
    for name in ('main_nac', 'c64', 'c1', 'ident'):
        inp, ref = R.case(name)
        _same(hostcheck(inp['logits'], inp['keys'], inp['size'], inp['align'], program=exe), ref)
    inp, ref = R.case('main_ac')
    valid = np.ones((3,) + inp['size'], dtype=np.float32)
    valid[2] = 0.0
    _same(hostcheck(inp['logits'], inp['keys'], inp['size'], True, valid, program=exe),
          R.classmix(inp['logits'], inp['keys'], inp['size'], True, valid))
    rng = np.random.RandomState(9)
    for n, H, W in ((5, 1, 3), (3, 1, 1), (2, 1, 1025)):                       # heads and tails of the 16-byte groups
        logits = rng.standard_normal((n, 4, 2, 2)).astype(np.float32)
        got = hostcheck(logits, rng.random_sample((n, 4)), (H, W), True, program=exe)
        assert got['pred'].max() < 4 and set(np.unique(got['mask']).tolist()) <= {0.0, 1.0}
