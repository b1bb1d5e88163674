"""
CPU-only: cross pseudo supervision without a GPU.

  * the new ABI symbol: declared, exported, prototyped, version 101; the descriptor's layout in C; every CMS_EINVAL case
    (decided before any HIP call)
  * ops.cps_labels' refusals; CrossPseudoStep's refusal of more than one process
  * the command line of train_seg_semisup_cps: the CutMix trainer's with six options removed and two defaults changed; its refusals, which come before the GPU
  * the margins of the cases the host-driver and GPU tests share (tests/_cps_refs.py), and properties of the restatement itself
(csrc/cps_math.hpp driven on the host is tests/test_cps_hostcheck.py)
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
import _hostcheck
import _cps_refs as R


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbol_is_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+cms_cps_labels\s*\(const cms_cps_desc\* d, void\* stream\);', header)
    assert hasattr(_lib.lib, 'cms_cps_labels') and 'cms_cps_labels' in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['cms_cps_labels'] == (ctypes.c_int, [ctypes.POINTER(_lib.CpsDesc), ctypes.c_void_p])
    assert _lib.version() == 101 and '#define CMS_VERSION 101' in header


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    fields = [name for name, _ in _lib.CpsDesc._fields_]
    assert fields == ['l0_a', 'l1_a', 'l0_b', 'l1_b', 'ranges', 'mask', 'um0', 'um1', 'n', 'c', 'h', 'w', 'H', 'W', 'align_corners',
                      'n_boxes', 'invert', 'conf_thresh', 'label_a', 'label_b', 'stats']
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu", sizeof(cms_cps_desc));\n'
            + ''.join('printf(" %zu", offsetof(cms_cps_desc, {}));\n'.format(f) for f in fields) + 'return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.CpsDesc
    assert sizes == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


def _desc(**over):
    """a descriptor cms_cps_labels would accept (host pointers: never dereferenced before the launch), then `over`"""
    from cutmix_semisup_seg_amd import _lib
    buf = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    d = _lib.CpsDesc()
    d.l0_a, d.l1_a, d.l0_b, d.l1_b, d.mask, d.um0, d.um1, d.label_a, d.label_b, d.stats = (p,) * 10
    d.n, d.c, d.h, d.w, d.H, d.W, d.align_corners, d.n_boxes, d.invert = 1, 3, 2, 2, 4, 4, 1, 0, 1
    d._keep = buf
    for key, val in over.items():
        setattr(d, key, val)
    return d


BAD = [
    ('logits NULL', dict(l0_a=None)), ('logits NULL', dict(l1_a=None)), ('logits NULL', dict(l0_b=None)), ('logits NULL', dict(l1_b=None)),
    ('label output NULL', dict(label_a=None)), ('label output NULL', dict(label_b=None)), ('stats NULL', dict(stats=None)),
    ('num_classes', dict(c=0)), ('num_classes', dict(c=65)), ('num_classes', dict(c=-3)),
    ('geometry', dict(n=0)), ('geometry', dict(n=-1)), ('geometry', dict(h=0)), ('geometry', dict(w=-2)), ('geometry', dict(H=0)),
    ('geometry', dict(W=-1)),
    ('65535', dict(n=65536, h=1, w=1, H=1, W=1)),
    ('h <= H', dict(h=5)), ('h <= H', dict(w=5)),
    ('2^31 - 1 output', dict(n=2, H=2 ** 15, W=2 ** 15)), ('2^31 - 1 output', dict(n=1, H=2 ** 31 - 1, W=2 ** 31 - 1)),
    ('2^31 - 1 logits', dict(c=64, h=2 ** 13, w=2 ** 13, H=2 ** 13, W=2 ** 13)),
    ('exactly one of ranges / mask', dict(mask=None)),
    ('n_boxes', dict(mask=None, ranges='p', n_boxes=0)),
]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f = _lib.fn['cms_cps_labels']
    assert f(None, None) == -1 and b'NULL descriptor' in _lib.fn['cms_last_error']()
    for what, over in BAD:
        d = _desc()
        over = {k: (d.stats if v == 'p' else v) for k, v in over.items()}
        d = _desc(**over)
        assert f(ctypes.byref(d), None) == -1, over
        assert what.encode() in _lib.fn['cms_last_error'](), (over, _lib.fn['cms_last_error']())
    d = _desc()
    d.ranges = d.mask                                                       # both
    d.n_boxes = 1
    assert f(ctypes.byref(d), None) == -1 and b'exactly one of ranges / mask' in _lib.fn['cms_last_error']()
    d = _desc()
    d.stats = d.stats + 4
    assert f(ctypes.byref(d), None) == -1 and b'aligned' in _lib.fn['cms_last_error']()
    with pytest.raises(ValueError, match='cps_labels'):
        _lib.check(f(ctypes.byref(_desc(c=65)), None), 'cms_cps_labels')
    # (that um0 and um1 may be NULL is tests/test_gpu_cps.py's to show: an accepted descriptor launches)


def test_ops_check_their_arguments_before_the_library():
    import torch
    from cutmix_semisup_seg_amd import ops
    lg = torch.zeros(2, 3, 4, 4)
    mask = torch.zeros(2, 1, 8, 8)
    ranges = torch.zeros(2, 1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.cps_labels(lg, lg, lg, lg, (8, 8), mask=mask)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.cps_labels(lg, lg, lg, lg, (8, 8), ranges=ranges)
    for exc, call in (
            (ValueError, lambda: ops.cps_labels(lg, lg, lg, lg, (8, 8))),                                    # neither
            (ValueError, lambda: ops.cps_labels(lg, lg, lg, lg, (8, 8), ranges=ranges, mask=mask)),          # both
            (ValueError, lambda: ops.cps_labels(lg, lg, lg, lg[:, :2], (8, 8), mask=mask)),
            (ValueError, lambda: ops.cps_labels(lg, lg, lg, lg, (3, 8), mask=mask)),                         # h > H
            (ValueError, lambda: ops.cps_labels(lg, lg, lg, lg, (0, 8), mask=mask)),
            (ValueError, lambda: ops.cps_labels(*[torch.zeros(1, 65, 2, 2)] * 4, (8, 8), mask=mask)),
            (TypeError, lambda: ops.cps_labels(lg, lg, lg, lg, 8, mask=mask)),
            (TypeError, lambda: ops.cps_labels(lg, lg, lg, lg[0], (8, 8), mask=mask))):
        with pytest.raises(exc):
            call()


def test_step_refuses_more_than_one_process(monkeypatch):
    from cutmix_semisup_seg_amd.cps import CrossPseudoStep, CPSConfig
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='runs on one GPU: data-parallel CPS'):
        CrossPseudoStep(object(), object(), None, None, CPSConfig())
    monkeypatch.setenv('WORLD_SIZE', '1')
    net = object()
    with pytest.raises(ValueError, match='one object'):
        CrossPseudoStep(net, net, None, None, CPSConfig())
    cfg = CPSConfig()
    assert cfg.cons_weight == 1.5 and cfg.conf_thresh == 0.0 and cfg.invert


# ------------------------------------------------------------------------------------------------------------------ command
def _table(command):
    return [(p.name, type(p.type).__name__, p.default, getattr(p, 'is_flag', False)) for p in command.params]


def test_option_table_is_the_cutmix_trainers_with_the_listed_changes():
    import train_seg_semisup_mask_mt as cutmix
    import train_seg_semisup_cps as cps
    base = _table(cutmix.experiment)
    gone = ['model', 'teacher_alpha', 'cons_loss_fn', 'conf_per_pixel', 'no_fuse_batches', 'allreduce_dtype']
    assert all(any(t[0] == g for t in base) for g in gone)
    changed = {'cons_weight': 1.5, 'conf_thresh': 0.0}
    want = [((t[0], t[1], changed[t[0]], t[3]) if t[0] in changed else t) for t in base if t[0] not in gone]
    got = _table(cps.experiment)
    assert [t[0] for t in got] == [t[0] for t in want] and len(got) == len(base) - 6
    assert got == want                                               # every other option keeps its type and default
    mode = [p for p in cps.experiment.params if p.name == 'mask_mode'][0]
    assert list(mode.type.choices) == ['mix'] and mode.default == 'mix'
    assert cps.train_seg_semisup_cps is not None
    # the CutMix trainer's own table is what it was
    assert dict((t[0], t[2]) for t in base)['cons_weight'] == 1.0 and dict((t[0], t[2]) for t in base)['conf_thresh'] == 0.97


def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_command_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_cps as cps
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    base = ['--synthetic', '--crop_size', '33,33']
    for n, extra in enumerate((['--mask_mode', 'zero'], ['--model', 'pi'], ['--teacher_alpha', '0.9'], ['--cons_loss_fn', 'var'],
                               ['--conf_per_pixel'], ['--no_fuse_batches'], ['--allreduce_dtype', 'bf16'])):
        res = CliRunner().invoke(cps.experiment, base + ['--job_desc', 'r{}'.format(n)] + extra)
        assert res.exit_code == 2 and not isinstance(res.exception, AssertionError), (extra, res.output, res.exception)
    res = CliRunner().invoke(cps.experiment, base + ['--job_desc', 's', '--synthetic_source_size', '64'])
    assert isinstance(res.exception, ValueError) and 'synthetic_source_size' in str(res.exception)
    res = CliRunner().invoke(cps.experiment, ['--job_desc', 'c', '--synthetic', '--crop_size', ''])
    assert isinstance(res.exception, ValueError) and '--crop_size' in str(res.exception)
    monkeypatch.setenv('WORLD_SIZE', '2')
    res = CliRunner().invoke(cps.experiment, base + ['--job_desc', 'w'])
    assert isinstance(res.exception, RuntimeError) and 'runs on one GPU: data-parallel CPS is not implemented' in str(res.exception)
    monkeypatch.delenv('WORLD_SIZE')
    # with everything in order the program gets as far as the GPU, and only there is it stopped
    res = CliRunner().invoke(cps.experiment, base + ['--job_desc', 'ok'])
    assert isinstance(res.exception, AssertionError) and 'the GPU was touched' in str(res.exception)


def test_run_epochs_takes_an_optional_after_epoch_hook():
    import inspect
    from cutmix_semisup_seg_amd import trainer_common as tc
    assert inspect.signature(tc.run_epochs).parameters['after_epoch'].default is None


# ------------------------------------------------------------------------------------------------------------------ the cases
CASES = [(name, align, kind) for name in R.GEOMETRIES for align in (True, False) for kind in R.KINDS]

# the seeds a CPU search of the float-mask recipe found before the code existed (align_corners True / False): this draw reproduces them
FIRST_SEEDS = {'main': (15, 14), 'c21': (11, 11), 'ident': (11, 11), 'one': (11, 11), 'c64': (12, 11), 'tab2c19': (13, 12)}


@pytest.mark.parametrize('name,align,kind', CASES, ids=lambda v: str(v))
def test_case_margins(name, align, kind):
    """The condition on the INPUTS of the shared cases: no near-tie and no confidence near the threshold at any pixel."""
    inp = R.case(name, align, kind)
    ref = R.reference(name, align, kind, False, R.TAU)
    n, c = inp['logits'][0].shape[:2]
    share = ref['stats'][1:3] / ref['stats'][0]
    print(name, align, kind, 'gap', ref['gap'], 'conf margin', ref['conf_margin'], 'kept', share, 'mix', inp['m'].mean())
    assert ref['gap'] >= R.GAP and ref['conf_margin'] >= R.CONF
    assert R.reference(name, align, kind, True, 0.0)['gap'] >= R.GAP
    if kind == 'rand':
        assert R.SEEDS[(name, align, kind)] == FIRST_SEEDS[name][0 if align else 1]
        assert R.search(name, align, kind) == R.SEEDS[(name, align, kind)]                # the FIRST seed from 11 upwards
        if name != 'one':
            assert (share > 0.02).all() and (share < 0.95).all()                          # the threshold decides something
    assert ref['stats'][3] <= ref['stats'][0] and (c > 5 or ref['stats'][3] > 0)          # few classes: the networks agree somewhere
    with_um = R.reference(name, align, kind, True, R.TAU)
    assert 0 < with_um['stats'][0] < ref['stats'][0]                                      # and so do the validity maps
    if name == 'tab2c19':
        assert inp['size'][0] * inp['size'][1] > 2 * 1024                                 # several workgroups per sample


def test_box_masks_are_the_parity_of_the_boxes():
    ranges = np.array([[[1, 4, 2, 6], [3, 8, 0, 3]], [[0, 0, 0, 0], [2, 3, 2, 3]]], dtype=np.int32)
    m = R.box_mask(ranges, (8, 7), True)
    assert m[0, 1, 2] and m[0, 3, 5] and not m[0, 3, 2] and m[0, 7, 0] and not m[0, 0, 0]        # (3, 2) lies in both boxes
    assert m[1].sum() == 1 and m[1, 2, 2]
    assert np.array_equal(R.box_mask(ranges, (8, 7), False), ~m)


def test_reference_properties():
    inp = R.case('main', True, 'rand')
    lg, size = inp['logits'], inp['size']
    ref = R.cps_labels(*lg, size, True, inp['m'], inp['um0'], inp['um1'], R.TAU)
    # the two networks swapped: the maps and their counts swap, the agreement stays
    sw = R.cps_labels(lg[2], lg[3], lg[0], lg[1], size, True, inp['m'], inp['um0'], inp['um1'], R.TAU)
    assert np.array_equal(sw['label_a'], ref['label_b']) and sw['stats'].tolist() == ref['stats'][[0, 2, 1, 3]].tolist()
    # the images swapped under the complementary mask: nothing changes
    co = R.cps_labels(lg[1], lg[0], lg[3], lg[2], size, True, ~inp['m'], inp['um1'], inp['um0'], R.TAU)
    assert np.array_equal(co['label_a'], ref['label_a']) and co['stats'].tolist() == ref['stats'].tolist()
    # a network against itself agrees everywhere; a constant mask reads one image only
    me = R.cps_labels(lg[0], lg[1], lg[0], lg[1], size, True, inp['m'])
    assert me['stats'][3] == me['stats'][0] == inp['m'].size and np.array_equal(me['label_a'], me['label_b'])
    ones = R.cps_labels(*lg, size, True, np.ones_like(inp['m']))
    assert np.array_equal(ones['label_a'], R.T.upsample(lg[1], size, True).argmax(1))
    # a sample alone is the sample in its batch
    one = R.cps_labels(*[t[1:2] for t in lg], size, True, inp['m'][1:2], inp['um0'][1:2], inp['um1'][1:2], R.TAU)
    assert np.array_equal(one['label_a'][0], ref['label_a'][1]) and np.array_equal(one['label_b'][0], ref['label_b'][1])
