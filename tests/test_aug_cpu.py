"""
CPU-only checks of the augmentation mean-teacher trainer's host surface: the reference restatement's own error budget, the
theta -> pixel-matrix fold, the pair geometry (aug_pairs.py) against matrices written by the reference's datapipe/affine.py
(tests/golden/aug_pairs.json) and against views actually cut from an image, the C ABI, the command line against the
reference's (tests/golden/aug_cli.json; both fixtures are written by tests/golden/make_aug_golden.py), and the staged / global
route every geometry of tests/test_gpu_aug.py reaches.
"""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, load_golden_json
import _hostcheck
import _aug_refs as refs

AUG_SYMBOLS = ('cms_aug_workspace_bytes', 'cms_aug_fwd', 'cms_aug_bwd')


# ---------------------------------------------------------------------------------------------------------------- reference
def numpy_warp(img, A):
    """(N,C,H,W) float64 sampled at the pixel-space positions A (N,6): four taps, zero padding -- written out with numpy,
    independent of F.affine_grid / F.grid_sample"""
    N, C, H, W = img.shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros_like(img)
    for n in range(N):
        a = A[n].astype(np.float64)
        ix, iy = a[0] * xs + a[1] * ys + a[2], a[3] * xs + a[4] * ys + a[5]
        x0, y0 = np.floor(ix), np.floor(iy)
        for dy in (0, 1):
            for dx in (0, 1):
                X, Y = (x0 + dx).astype(int), (y0 + dy).astype(int)
                wgt = (1 - np.abs(ix - (x0 + dx))) * (1 - np.abs(iy - (y0 + dy)))
                ok = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
                out[n] += np.where(ok, wgt, 0.0) * img[n][:, np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)]
    return out


THETAS = [refs.rot_scale_theta(17, 1.0, 0.05, -0.03), refs.rot_scale_theta(-33, 1.3), refs.rot_scale_theta(5, 0.8, -0.1, 0.08)]


def test_pixel_matrix_fold_gives_the_grid_sample_coordinates():
    """ops.aug_pixel_matrices folds F.affine_grid(align_corners=True) and grid_sample's un-normalisation: a numpy sampler driven
    by the folded matrices reproduces torch's own affine_grid + grid_sample in float64; and the fold inverts exactly"""
    from cutmix_semisup_seg_amd import ops
    H, W = 23, 37
    gen = torch.Generator().manual_seed(2)
    img = torch.randn(3, 4, H, W, generator=gen, dtype=torch.float64)
    theta = torch.tensor(THETAS, dtype=torch.float64)
    want = F.grid_sample(img, F.affine_grid(theta, list(img.shape), align_corners=True), align_corners=True)
    A64 = refs.theta_from_pixel_affine  # (its inverse below)
    rx, ry = (W - 1) / 2.0, (H - 1) / 2.0
    t = theta.numpy()
    A = np.stack([t[:, 0, 0], t[:, 0, 1] * rx / ry, (t[:, 0, 2] - t[:, 0, 0] - t[:, 0, 1] + 1) * rx,
                  t[:, 1, 0] * ry / rx, t[:, 1, 1], (t[:, 1, 2] - t[:, 1, 0] - t[:, 1, 1] + 1) * ry], axis=1)
    np.testing.assert_allclose(numpy_warp(img.numpy(), A), want.numpy(), rtol=0, atol=1e-12)
    got = ops.aug_pixel_matrices(theta, (H, W))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 6)
    np.testing.assert_array_equal(got.numpy(), A.astype(np.float32))               # float64 fold, one rounding
    np.testing.assert_allclose(A64(A.reshape(3, 2, 3), H, W).numpy(), t, rtol=0, atol=1e-14)
    # numpy and float32 input are accepted alike; exact identity and flips stay exact
    np.testing.assert_array_equal(ops.aug_pixel_matrices(theta.numpy(), (H, W)).numpy(), got.numpy())
    eye = ops.aug_pixel_matrices(np.array([[[1, 0, 0], [0, 1, 0]], [[-1, 0, 0], [0, -1, 0]]], dtype=np.float32), (H, W))
    np.testing.assert_array_equal(eye.numpy(), [[1, 0, 0, 0, 1, 0], [-1, 0, W - 1, 0, -1, H - 1]])
    with pytest.raises(ValueError):
        ops.aug_pixel_matrices(theta, (1, W))
    with pytest.raises(ValueError):
        ops.aug_pixel_matrices(theta.reshape(3, 6), (H, W))


@pytest.mark.parametrize('mode', ['default', 'per_pixel', 'no_thresh'])
@pytest.mark.parametrize('fn', refs.LOSS_FNS)
def test_float32_restatement_stays_inside_a_quarter_of_the_tolerances(fn, mode):
    """The error budget behind the tolerances of the host check and the GPU tests (loss rel 2e-5, gradient rtol 5e-4 + atol
    5e-6 max|want|): the reference's own float32 arithmetic against the same statements in float64 at 3 x 21 x 9 x 19 -> 70 x
    150 uses well under a quarter of them, so the kernels are held to the reference's value, not to its rounding noise."""
    tau, pp = {'default': (0.6, False), 'per_pixel': (0.6, True), 'no_thresh': (0.0, False)}[mode]
    gen = torch.Generator().manual_seed(29)
    ls = torch.randn(3, 21, 9, 19, generator=gen) * 2
    lt = torch.randn(3, 21, 9, 19, generator=gen) * 3
    um0 = (torch.rand(3, 1, 70, 150, generator=gen) > 0.3).float()
    um1 = (torch.rand(3, 1, 70, 150, generator=gen) > 0.3).float()
    kw = dict(cons_loss_fn=fn, conf_thresh=tau, conf_per_pixel=pp, ramp_val=0.7, rampup=5, cons_weight=0.3)
    r32, g32, c32 = refs.aug_from_lowres(ls, lt, THETAS, um0, um1, (70, 150), True, **kw)
    r64, g64, c64 = refs.aug_from_lowres(ls, lt, THETAS, um0, um1, (70, 150), True, dtype=torch.float64, **kw)
    if tau > 0:
        assert float((c64 - tau).abs().min()) > 1e-5
        assert r32['conf_rate'] == pytest.approx(r64['conf_rate'], abs=0.25 * 2e-6)      # (a float32 mean of the same indicator)
    assert float(r32['unsup_loss'].detach()) == pytest.approx(float(r64['unsup_loss'].detach()), rel=0.25 * 2e-5)
    g64 = g64.numpy()
    excess = np.abs(g32.numpy() - g64) / (5e-4 * np.abs(g64) + 5e-6 * np.abs(g64).max())
    assert excess.max() < 0.25


# ---------------------------------------------------------------------------------------------------------------- pair geometry
def _case_matrices(ap, c):
    """the matrices of one recorded case from aug_pairs' helpers, composed as PairGeometry composes them"""
    p = c['params']
    crop = np.array(p['crop'])
    if 'pos0' in p:
        pos = np.array([p['pos0'][::-1], p['pos1'][::-1]])
        factors = np.append(np.array([[1, 1]]), crop[None, ::-1].astype(float) / np.array(p['size1'])[None, ::-1], axis=0)
        xf = ap.cat(ap.translation((factors - 1.0) * 0.5), ap.scaling(factors), ap.translation(-pos), ap.identity(2))
    else:
        centre = np.array([p['centre'], p['centre']])
        off = np.stack([np.zeros((2,)), np.array(p['offset1'])])
        xf = ap.cat(ap.translation(crop[None, ::-1] * 0.5), ap.translation(off[:, ::-1]), ap.rotation(np.array(p['thetas'])),
                    ap.scaling(np.array(p['scales'])[:, ::-1]), ap.translation(-centre[:, ::-1]))
    xf = ap.cat(ap.flips(np.array(p['flips']) != 0, tuple(crop)), xf)
    return xf, ap.xf0_to_1(xf[0:1], xf[1:2], tuple(crop))[0]


def test_pair_matrices_match_the_reference_affine_functions():
    """float32 matrices, composed in float32 in the reference's order: equal to what datapipe/affine.py wrote, to the last bit"""
    from cutmix_semisup_seg_amd import aug_pairs as ap
    cases = load_golden_json('aug_pairs')
    assert len(cases) == 7
    for c in cases:
        xf, t01 = _case_matrices(ap, c)
        assert xf.dtype == np.float32 and t01.dtype == np.float32
        np.testing.assert_array_equal(xf, np.array(c['xf_cv'], dtype=np.float32))
        np.testing.assert_array_equal(t01, np.array(c['xf0_to_1'], dtype=np.float32))


def _cut(img, pos, crop, flips):
    v = img[pos[0]:pos[0] + crop[0], pos[1]:pos[1] + crop[1]]
    if flips[0]:
        v = v[:, ::-1]
    if flips[1]:
        v = v[::-1]
    if flips[2]:
        v = v.swapaxes(0, 1)
    return np.ascontiguousarray(v)


@pytest.mark.parametrize('crop,hv', [((33, 41), False), ((40, 40), True)], ids=['33x41', '40x40_transpose'])
def test_xf0_to_1_warps_view0_onto_view1(crop, hv):
    """The convention end to end: two views cut from one image by integer crops and flips (the drawn positions and flags) satisfy
    grid_sample(view0, affine_grid(xf0_to_1)) == view1 wherever the warped all-ones mask is 1. The image holds integers 0..15 and
    the matrices are float32 (a translation such as 0.35 is not representable: the coordinates are off by up to ~2e-5 pixels),
    so 'equal' is: equal after rounding to the integer grid, and within 1e-3 before it."""
    from cutmix_semisup_seg_amd import aug_pairs as ap
    pg = ap.PairGeometry(crop, offset_range=16.0, hflip=True, vflip=True, hvflip=hv, rng=np.random.RandomState(3))
    seen = 0
    for it in range(8):
        img = np.random.RandomState(it).randint(0, 16, size=(60, 70)).astype(np.float64)
        xf, t01, info = pg.draw(img.shape)
        v0, v1 = _cut(img, info['pos0'], crop, info['flips'][0]), _cut(img, info['pos1'], crop, info['flips'][1])
        grid = F.affine_grid(torch.tensor(t01[None], dtype=torch.float64), [1, 1, crop[0], crop[1]], align_corners=True)
        warped = F.grid_sample(torch.tensor(v0[None, None]), grid, align_corners=True)[0, 0].numpy()
        mask = F.grid_sample(torch.ones(1, 1, *crop, dtype=torch.float64), grid, align_corners=True)[0, 0].numpy()
        inside = mask > 1 - 1e-4
        assert inside.sum() > 0.3 * crop[0] * crop[1]          # the views overlap (offsets of at most 16 pixels)
        np.testing.assert_array_equal(np.round(warped[inside]), v1[inside])
        assert np.abs(warped[inside] - v1[inside]).max() < 1e-3
        seen += int(info['flips'].any())
    assert seen > 0


def test_pair_draws_follow_the_transform_choice():
    """:129-144 -- Hung's scale crop wins over rotate / scale, which is chosen by max_scale != 1 or rot_mag != 0; the draws are
    reproducible from the RandomState and stay in range"""
    from cutmix_semisup_seg_amd import aug_pairs as ap
    kinds = {}
    for name, kw in dict(crop={}, hung=dict(scale_hung=True, max_scale=1.5, rot_mag=30.0), warp=dict(max_scale=1.5),
                         rot=dict(rot_mag=30.0, free_scale_rot=True, scale_non_uniform=True)).items():
        a = ap.PairGeometry((33, 41), rng=np.random.RandomState(7), **kw).draw_batch(4, (60, 70))
        b = ap.PairGeometry((33, 41), rng=np.random.RandomState(7), **kw).draw_batch(4, (60, 70))
        np.testing.assert_array_equal(a[0], b[0])
        assert a[0].shape == (4, 2, 3) and a[0].dtype == np.float32 and a[1].shape == (4, 2, 2, 3)
        kinds[name] = a[2][0]['kind']
        if name == 'rot':
            info = a[2][0]
            assert np.all(np.abs(info['thetas']) <= math.radians(30.0)) and info['thetas'][0] != info['thetas'][1]
            assert np.all(np.abs(info['offset1']) <= 16)
        if name == 'warp':
            info = a[2][0]
            assert info['thetas'][0] == info['thetas'][1] == 0.0 and np.all(info['scales_yx'][0] == info['scales_yx'][1])
            assert np.all((info['scales_yx'] >= 1 / 1.5) & (info['scales_yx'] <= 1.5))
    assert kinds == dict(crop='crop', hung='hung', warp='warp', rot='warp')
    with pytest.raises(ValueError):
        ap.PairGeometry((33, 41), hvflip=True)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_aug_symbols_at_the_same_abi_version():
    from cutmix_semisup_seg_amd import _lib
    header = open(os.path.join(REPO, 'include', 'cutmixseg.h')).read()
    for name in AUG_SYMBOLS:
        assert name + '(' in header, '{} is not declared in cutmixseg.h'.format(name)
        assert hasattr(_lib.lib, name), 'libcutmixseg_hip.so does not export {}'.format(name)
        assert name in _lib.PROTOTYPES
    assert _lib.version() == 101


def test_aug_desc_layout_matches_the_c_compiler():
    from cutmix_semisup_seg_amd import _lib
    fields = [f[0] for f in _lib.AugDesc._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) {\n'
    prog += '  printf("%zu\\n", sizeof(cms_aug_desc));\n'
    for f in fields:
        prog += '  printf("%zu\\n", offsetof(cms_aug_desc, {}));\n'.format(f)
    prog += '  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        out = [int(x) for x in subprocess.check_output([_hostcheck.compile_against_header(prog, d)]).decode().split()]
    assert out[0] == ctypes.sizeof(_lib.AugDesc)
    assert out[1:] == [getattr(_lib.AugDesc, f).offset for f in fields]


def test_bad_aug_arguments_come_back_as_error_codes():
    """Argument validation happens before any HIP call, so it is checkable without a GPU."""
    from cutmix_semisup_seg_amd import _lib
    fn = _lib.fn
    d = _lib.AugDesc()                                             # all NULL, all zero
    assert fn['cms_aug_fwd'](ctypes.byref(d), None, None, None) == -1
    assert b'NULL' in fn['cms_last_error']()
    assert fn['cms_aug_bwd'](ctypes.byref(d), None, None, None) == -1
    assert fn['cms_aug_fwd'](None, None, None, None) == -1
    assert fn['cms_aug_workspace_bytes'](None) == 0
    assert fn['cms_aug_workspace_bytes'](ctypes.byref(d)) == 0     # zero geometry
    # pointers that are never followed: the geometry is refused first
    d.l_stu = d.l_tea = 4096
    assert fn['cms_aug_fwd'](ctypes.byref(d), 4096, 4096, None) == -1
    assert b'xf' in fn['cms_last_error']()
    d.xf = 4096
    d.n, d.c, d.h, d.w, d.H, d.W = 2, 5, 6, 7, 0, 50
    assert fn['cms_aug_fwd'](ctypes.byref(d), 4096, 4096, None) == -1
    assert b'geometry' in fn['cms_last_error']()
    d.h, d.H = 1, 1                                                # the align_corners=True grid is undefined for one row
    assert fn['cms_aug_fwd'](ctypes.byref(d), 4096, 4096, None) == -1
    assert b'H >= 2' in fn['cms_last_error']()
    d.h, d.H = 6, 5                                                # logits larger than the loss geometry
    assert fn['cms_aug_fwd'](ctypes.byref(d), 4096, 4096, None) == -1
    d.H, d.loss_fn = 41, 7
    assert fn['cms_aug_bwd'](ctypes.byref(d), 4096, 4096, None) == -1
    assert b'Unknown consistency loss function' in fn['cms_last_error']()
    d.loss_fn = 0
    assert fn['cms_aug_fwd'](ctypes.byref(d), None, 4096, None) == -1          # no workspace
    assert fn['cms_aug_bwd'](ctypes.byref(d), None, 4096, None) == -1          # no scalars
    assert fn['cms_aug_workspace_bytes'](ctypes.byref(d)) == 2 * 1 * 6 * 3 * 4  # one tile column x 6 tile rows per sample


def test_aug_ops_refuse_cpu_tensors_and_unknown_losses():
    from cutmix_semisup_seg_amd import ops
    lo = torch.zeros(2, 5, 2, 2)
    xf = np.zeros((2, 2, 3), dtype=np.float32)
    with pytest.raises(ValueError, match='GPU'):
        ops.aug_consistency_forward(ops.AugConsistencyConfig(), lo, lo, xf, (4, 4))
    with pytest.raises(ValueError, match='Unknown consistency loss function'):
        ops.AugConsistencyConfig(loss_fn='l2')


# ---------------------------------------------------------------------------------------------------------------- trainer
def test_aug_cli_surface_matches_reference():
    import train_seg_semisup_aug_mt as trainer
    ref = load_golden_json('aug_cli')
    assert len(ref) == 51
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
    # what sets this trainer apart (train_seg_semisup_aug_mt.py:534, 542, 551)
    assert mine['cons_weight'].default == 1.0 and mine['aug_offset_range'].default == 16.0
    assert mine['aug_free_scale_rot'].is_flag and 'ict_alpha' not in mine


def test_aug_trainer_without_synthetic_is_refused(tmp_path, monkeypatch):
    """No dataset pipeline in this build: the job refuses to start, exits non-zero and leaves no log behind (job_helper.JobNotRun),
    as the other trainers do."""
    from click.testing import CliRunner
    import train_seg_semisup_aug_mt as trainer
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'nodata'])
    assert res.exit_code != 0
    assert 'run with --synthetic' in res.output + str(res.exception)
    assert not (tmp_path / 'results' / 'train_seg_semisup_aug_mt' / 'log_nodata.txt').exists()


def test_aug_step_refuses_data_parallel_runs(monkeypatch):
    from cutmix_semisup_seg_amd import aug
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='one GPU'):
        aug.AugMeanTeacherStep(None, None, None, None, aug.AugConfig())


# ---------------------------------------------------------------------------------------------------------------- tile facts
@pytest.fixture(scope='module')
def hc():
    return _hostcheck.load('hostcheck_aug')


def test_gpu_geometries_reach_the_routes_they_are_meant_to(hc):
    """The staged / global decision of the kernels (capacity rule of the host + per-workgroup rectangle), restated in
    tests/_aug_refs.py on the product's own aug_tile_box: which route each geometry of tests/test_gpu_aug.py takes."""
    from cutmix_semisup_seg_amd import ops
    import test_gpu_aug as gpu
    assert {g['C'] for g in gpu.GEOS.values() if g['lo'] == g['hi']} == {2, 3}     # identity kernels: compile-time and run-time C
    for name, g in sorted(gpu.GEOS.items()):
        if g['lo'] == g['hi']:
            assert refs.tea_capacity(g['C'], g['lo'], g['hi'], g['ac'], False) is None      # identity geometry: the direct kernels
            continue
        xf = ops.aug_pixel_matrices(np.asarray(g['theta']), g['hi']).numpy()
        if name == 'direct_rt':
            # the student's rectangle alone is beyond the forward limit: the direct forward kernel (run-time C); the backward is
            # tiled with what G, R and the student's rectangle leave for the teacher's -- too little for any of these tiles
            assert g['C'] not in (2, 5, 19, 21) and refs.tea_capacity(g['C'], g['lo'], g['hi'], g['ac'], False) is None
            f = refs.tile_facts(hc, xf, g['C'], g['lo'], g['hi'], g['ac'], True)
            assert 0 < f['cap'] < 32 * 1024 // 4 and f['staged'] == 0 and f['global_'] > 0, (name, f)
            continue
        for backward in (False, True):
            f = refs.tile_facts(hc, xf, g['C'], g['lo'], g['hi'], g['ac'], backward)
            assert f['cap'] == 32 * 1024 // 4                       # nothing else limits the capacity at these sizes
            if name == 'fallback':
                # 64 x 8 / 64 x 4 tiles at 45 degrees sample ~50 x 50 cells of 21 classes: ~200 KB against 32 KB
                assert f['staged'] == 0 and f['global_'] > 0 and f['max_floats'] * 4 > 150 * 1024, (name, f)
            else:
                assert f['staged'] > 0 and f['global_'] == 0, (name, f)
            if name.startswith('tiles'):
                assert f['outside'] > 0, (name, f)                  # wholly outside tiles of the third warp
    # the tile grids the geometry comments of test_gpu_aug.py describe
    assert (150 + 63) // 64 == 3 and 150 - 2 * 64 == 22 and 70 % 8 == 6 and 70 % 4 == 2


def test_capacity_rule_at_the_sizes_of_the_design_note(hc):
    """Pascal scale (41 x 41 -> 321 x 321, C = 21): a tile rotated by 45 degrees and a further scale of 2 are staged; strong
    scales with many classes are not; a student rectangle beyond the forward limit leaves the tiled kernel altogether."""
    from cutmix_semisup_seg_amd import ops
    for theta, staged in ((refs.rot_scale_theta(45, 1.0), True), (refs.rot_scale_theta(45, 2.0), True)):
        xf = ops.aug_pixel_matrices(np.asarray([theta]), (321, 321)).numpy()
        for backward in (False, True):
            f = refs.tile_facts(hc, xf, 21, (41, 41), (321, 321), True, backward)
            assert (f['global_'] == 0) == staged and f['staged'] > 0, f
    assert refs.tea_capacity(21, (60, 60), (64, 64), True, False) == 8192
    assert refs.tea_capacity(64, (60, 60), (64, 64), True, False) is None           # 64 x 9 x 62 floats > 96 KB
