"""
CPU-only checks of the ICT trainer's host surface: the C ABI (symbols, struct layout, argument validation), the tensor
wrappers' refusal of CPU tensors, and the trainer's command line against the reference's (tests/golden/ict_cli.json, written
by tests/golden/make_ict_golden.py from the reference's own click command).
"""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import REPO, load_golden_json
import _hostcheck

ICT_SYMBOLS = ('cms_ict_blend', 'cms_ict_workspace_bytes', 'cms_ict_fwd', 'cms_ict_bwd')


def test_library_exports_the_ict_symbols_at_the_same_abi_version():
    from cutmix_semisup_seg_amd import _lib
    header = open(os.path.join(REPO, 'include', 'cutmixseg.h')).read()
    for name in ICT_SYMBOLS:
        assert name + '(' in header, '{} is not declared in cutmixseg.h'.format(name)
        assert hasattr(_lib.lib, name), 'libcutmixseg_hip.so does not export {}'.format(name)
        assert name in _lib.PROTOTYPES
    assert _lib.version() == 101


def test_ict_desc_layout_matches_the_c_compiler():
    from cutmix_semisup_seg_amd import _lib
    fields = [f[0] for f in _lib.IctDesc._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) {\n'
    prog += '  printf("%zu\\n", sizeof(cms_ict_desc));\n'
    for f in fields:
        prog += '  printf("%zu\\n", offsetof(cms_ict_desc, {}));\n'.format(f)
    prog += '  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        out = [int(x) for x in subprocess.check_output([_hostcheck.compile_against_header(prog, d)]).decode().split()]
    assert out[0] == ctypes.sizeof(_lib.IctDesc)
    assert out[1:] == [getattr(_lib.IctDesc, f).offset for f in fields]


def test_bad_ict_arguments_come_back_as_error_codes():
    """Argument validation happens before any HIP call, so it is checkable without a GPU."""
    from cutmix_semisup_seg_amd import _lib
    fn = _lib.fn
    d = _lib.IctDesc()                                             # all NULL, all zero
    assert fn['cms_ict_fwd'](ctypes.byref(d), None, None, None) == -1
    assert b'NULL' in fn['cms_last_error']()
    assert fn['cms_ict_bwd'](ctypes.byref(d), None, None, None, None) == -1
    assert fn['cms_ict_fwd'](None, None, None, None) == -1
    assert fn['cms_ict_workspace_bytes'](None) == 0
    assert fn['cms_ict_workspace_bytes'](ctypes.byref(d)) == 0     # zero geometry
    # pointers that are never followed: the geometry is refused first
    d.l_stu = d.l_tea0 = d.l_tea1 = d.lam = 4096
    d.n, d.c, d.h, d.w, d.H, d.W = 2, 5, 6, 7, 0, 50
    assert fn['cms_ict_fwd'](ctypes.byref(d), 4096, 4096, None) == -1
    assert b'geometry' in fn['cms_last_error']()
    d.H = 5                                                        # logits larger than the loss geometry
    assert fn['cms_ict_fwd'](ctypes.byref(d), 4096, 4096, None) == -1
    d.H, d.loss_fn = 41, 7
    assert fn['cms_ict_bwd'](ctypes.byref(d), 4096, 4096, 4096, None) == -1
    assert b'Unknown consistency loss function' in fn['cms_last_error']()
    d.loss_fn = 0
    assert fn['cms_ict_fwd'](ctypes.byref(d), None, 4096, None) == -1          # no workspace
    d.conf_thresh, d.conf_per_pixel = 0.5, 1
    assert fn['cms_ict_bwd'](ctypes.byref(d), None, 4096, 4096, None) == -1    # the confidence map lives in the workspace
    # the workspace grows by the (H,W) map in per-pixel mode only
    with_map = fn['cms_ict_workspace_bytes'](ctypes.byref(d))
    d.conf_per_pixel = 0
    assert with_map - fn['cms_ict_workspace_bytes'](ctypes.byref(d)) == 41 * 50 * 4
    # blend
    assert fn['cms_ict_blend'](None, None, None, 0, None, 1, 4, None) == -1
    assert fn['cms_ict_blend'](4096, 4096, 4096, 2, 4096, 1, 4, None) == -1    # unknown dtype
    assert fn['cms_ict_blend'](4096, 4096, 4096, 0, 4096, 0, 4, None) == -1
    with pytest.raises(ValueError):
        _lib.check(-1, 'cms_ict_blend')


def test_ict_ops_refuse_cpu_tensors():
    import torch
    from cutmix_semisup_seg_amd import ops
    x = torch.zeros(2, 3, 4, 4)
    lam = torch.zeros(2)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.ict_blend(x, x, lam)
    cfg = ops.ICTConsistencyConfig()
    lo = torch.zeros(2, 5, 2, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.ict_consistency_forward(cfg, lo, lo, lo, lam, (4, 4))
    with pytest.raises(ValueError, match='Unknown consistency loss function'):
        ops.ICTConsistencyConfig(loss_fn='l2')


def test_ict_cli_surface_matches_reference():
    import train_seg_semisup_ict as trainer
    ref = load_golden_json('ict_cli')
    assert len(ref) == 50
    mine = {p.name: p for p in trainer.experiment.params}
    for o in ref:
        assert o['name'] in mine, 'missing option --{}'.format(o['name'])
        p = mine[o['name']]
        assert list(p.opts) == o['opts']
        assert bool(getattr(p, 'is_flag', False)) == o['is_flag']
        assert type(p.type).__name__ == o['type'], o['name']
        assert p.default == o['default'] or str(p.default) == str(o['default']), o['name']
        if o['choices'] is not None:
            assert list(p.type.choices) == o['choices']
    assert [p.name for p in trainer.experiment.params][:len(ref)] == [o['name'] for o in ref]
    assert set(mine) - {o['name'] for o in ref} == {'synthetic', 'synthetic_n_classes', 'synthetic_val_batches',
                                                     'compute_dtype'}
    # the defaults that differ from the other two trainers (train_seg_semisup_ict.py:517, 541-543)
    assert mine['cons_weight'].default == 0.3 and mine['sgd_nesterov'].default is True and mine['ict_alpha'].default == 0.1
    assert list(mine['cons_loss_fn'].type.choices) == ['var', 'bce', 'kld', 'logits_var', 'logits_smoothl1']


def test_ict_trainer_without_synthetic_is_refused(tmp_path, monkeypatch):
    """No dataset pipeline in this build: the job refuses to start, exits non-zero and leaves no log behind (job_helper.JobNotRun),
    as the other trainers do."""
    from click.testing import CliRunner
    import train_seg_semisup_ict as trainer
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'nodata'])
    assert res.exit_code != 0
    assert 'run with --synthetic' in res.output + str(res.exception)
    assert not (tmp_path / 'results' / 'train_seg_semisup_ict' / 'log_nodata.txt').exists()


def test_ict_step_refuses_data_parallel_runs(monkeypatch):
    from cutmix_semisup_seg_amd import ict
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='one GPU'):
        ict.ICTMeanTeacherStep(None, None, None, None, ict.ICTConfig())


def test_gpu_geometries_reach_the_routes_they_are_meant_to():
    """Which forward / backward kernels each geometry of tests/test_gpu_ict.py runs (three staged rectangles, as the consistency:
    tests/_loss_refs.tile_facts), with a compile-time (2, 5, 19, 21) and a run-time class count on every route."""
    import _loss_refs as L
    import test_gpu_ict as gpu
    want = {'tiles_align': 'tiled', 'tiles_noalign': 'tiled', 'c5': 'tiled', 'c7': 'tiled', 'ident': 'identity',
            'ident_rt': 'identity', 'direct': 'direct', 'direct_rt': 'direct'}
    assert sorted(want) == sorted(gpu.GEOS)
    seen = set()
    for name, g in gpu.GEOS.items():
        f = L.tile_facts(g['C'], g['lo'][0], g['lo'][1], g['hi'][0], g['hi'][1], g['ac'], 3)
        assert f['forward'].replace('_optin', '') == want[name], (name, f)
        assert f['backward'].replace('_optin', '') == ('identity' if want[name] == 'identity' else 'tiled'), (name, f)
        seen.add((want[name], g['C'] in (2, 5, 19, 21)))
    assert seen == {(r, ct) for r in ('tiled', 'identity', 'direct') for ct in (True, False)}
    f = L.tile_facts(16, 60, 60, 64, 64, True, 3)
    assert f['fwd_lds'] == 3 * 16 * 9 * 62 * 4 > L.FWD_PATCH_LDS_MAX >= L.tile_facts(14, 60, 60, 64, 64, True, 3)['fwd_lds']
