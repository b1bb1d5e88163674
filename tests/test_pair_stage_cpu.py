"""
CPU: pairs of views for the augmentation trainer's data set path.

  * aug_pairs.pair_rows against PairGeometry's own matrices: the map output pixel -> source position a row implies is the inverse
    of xf_cv[v] at the four crop corners, to 1e-4 source pixels (the figure _stage_cases.ROUNDING_MARGIN uses);
  * the restated reference alone is self-consistent: both views staged by oracle/augment.py from those rows, view 0 warped into
    view 1 with xf0_to_1 (the reference's own commented-out debugging check, train_seg_semisup_aug_mt.py:315-338), on ramp
    sources, within 1.5 grey levels (tests/_pair_cases.compare_views says why);
  * a ragged draw equals the sequential single-pair draws;
  * the mask mode (params slot 23) of csrc/stage_math.hpp, driven on the host by tests/hostcheck_stage_pair over the ragged pool
    of tests/_stage_cases.py;
  * the refusals of the three trainers' data set path come before the GPU is touched.

The kernels are covered by tests/test_gpu_pair_stage.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden_json
import _hostcheck
import _pair_cases as pc
import _pascal_tree
import _stage_cases as sc

TRAINERS = ['train_seg_semisup_ict', 'train_seg_semisup_vat_mt', 'train_seg_semisup_aug_mt']


def _draw(name):
    from cutmix_semisup_seg_amd import aug_pairs
    crop, src_hw, cfg = pc.SELF_CONSISTENCY[name]
    geo = pc.make_geometry(crop, cfg, pc.SEED)
    xf01, xf_cv, infos = geo.draw_batch(pc.N_PAIRS, src_hw)
    rows = np.stack([aug_pairs.pair_rows(info, crop) for info in infos], axis=1)          # (2, n, 24), view-major
    return crop, src_hw, cfg, xf01, xf_cv, infos, rows


@pytest.mark.parametrize('name', list(pc.SELF_CONSISTENCY))
def test_rows_agree_with_the_matrices(name):
    from cutmix_semisup_seg_amd import aug_pairs
    crop, src_hw, cfg, xf01, xf_cv, infos, rows = _draw(name)
    assert rows.dtype == np.float32 and rows.shape == (2, pc.N_PAIRS, 24)
    pc.assert_pair_branches_covered(cfg, rows, crop)
    assert (rows[:, :, 7:10] == 1).all() and not rows[:, :, 10:15].any()                   # no colour change in pair_rows
    H, W = crop
    worst = 0.0
    for i in range(pc.N_PAIRS):
        inv = aug_pairs.inverse(xf_cv[i].astype(np.float64))                               # view v -> source, flips included
        for v in range(2):
            for ox, oy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
                want = inv[v] @ np.array([ox, oy, 1.0])
                got = pc.row_source_position(rows[v, i], crop, ox, oy)
                worst = max(worst, float(np.abs(np.array(got) - want).max()))
    print('{}: largest distance {:.3g} source pixels'.format(name, worst))
    assert worst <= sc.ROUNDING_MARGIN
    # the matrices kept in the parameters are the ones before the flips
    if not any(cfg.get(k) for k in ('hflip', 'vflip', 'hvflip')):
        assert all(np.array_equal(info['xf_cv'], xf_cv[i]) for i, info in enumerate(infos))


@pytest.fixture(scope='module')
def oracle_pairs():
    """Both views of every pair of every configuration, staged by the oracle once: name -> (image0, image1, mask0, mask1, xf0_to_1)"""
    out = {}
    for name in pc.SELF_CONSISTENCY:
        crop, src_hw, cfg, xf01, xf_cv, infos, rows = _draw(name)
        src = pc.ramp_source(src_hw)
        views = [[pc.oracle_view(src, rows[v, i], crop, np.zeros(3), np.ones(3)) for i in range(pc.N_PAIRS)] for v in range(2)]
        img = [torch.from_numpy(np.stack([o[0] for o in views[v]])) for v in range(2)]
        msk = [torch.from_numpy(np.stack([o[2] for o in views[v]]))[:, None] for v in range(2)]
        out[name] = (img[0], img[1], msk[0], msk[1], xf01)
    return out


@pytest.mark.parametrize('name', list(pc.SELF_CONSISTENCY))
def test_restated_reference_is_self_consistent(oracle_pairs, name):
    image0, image1, mask0, mask1, xf01 = oracle_pairs[name]
    if 'hung' in name:
        assert set(np.unique(mask1.numpy()).tolist()) <= {0.0, 1.0}                        # INTER_NEAREST of the mask
    worst, share = pc.compare_views(image0, image1, mask0, mask1, xf01)
    print('{}: worst difference {:.2f} levels, smallest share compared {:.1%}'.format(name, worst.max(), share.min()))
    assert share.min() >= pc.MIN_COMPARED, share
    assert worst.max() <= pc.MAX_LEVELS, worst


def test_a_shifted_view_fails_the_self_consistency_bound(oracle_pairs):
    """The check has teeth: view 1 moved by half a source pixel is far outside the bound."""
    crop, src_hw, cfg, xf01, xf_cv, infos, rows = _draw('plain')
    image0, image1, mask0, mask1, _ = oracle_pairs['plain']
    src = pc.ramp_source(src_hw)
    moved = rows[1].copy()
    moved[:, 15], moved[:, 22] = 1.0, 1.0
    for i in range(pc.N_PAIRS):                                                            # the same window as a warp, + (0.5, 0.5)
        moved[i, 16:22] = (1.0, 0.0, rows[1, i, 1] + 0.5, 0.0, 1.0, rows[1, i, 0] + 0.5)
    img1 = torch.from_numpy(np.stack([pc.oracle_view(src, moved[i], crop, np.zeros(3), np.ones(3))[0] for i in range(pc.N_PAIRS)]))
    worst, _ = pc.compare_views(image0, img1, mask0, mask1, xf01)
    assert worst.min() > pc.MAX_LEVELS


@pytest.mark.parametrize('cfg', [dict(), dict(scale_hung=True, hflip=True), dict(rot_mag=30.0, max_scale=1.5, free_scale_rot=True,
                                                                                  vflip=True)], ids=['crop', 'hung', 'warp'])
def test_a_ragged_draw_is_the_sequential_draws(cfg):
    sizes = [(1, 1), (37, 53), (20, 90), (20, 90), (60, 70), (90, 20), (5, 3), (48, 64)]
    xf01, xf_cv, infos = pc.make_geometry((48, 64), cfg, 9).draw_batch(len(sizes), sizes)
    one_by_one = pc.make_geometry((48, 64), cfg, 9)
    for i, s in enumerate(sizes):
        xf, x01, info = one_by_one.draw(s)
        assert np.array_equal(xf, xf_cv[i]) and np.array_equal(x01, xf01[i]) and info.keys() == infos[i].keys()
        assert all(np.array_equal(info[k], infos[i][k]) for k in info)
    assert len({tuple(x.ravel()) for x in xf01}) > 1
    # one size for the whole batch is unchanged
    a = pc.make_geometry((48, 64), cfg, 9).draw_batch(3, (60, 70))
    b = pc.make_geometry((48, 64), cfg, 9).draw_batch(3, [(60, 70)] * 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        pc.make_geometry((48, 64), cfg, 9).draw_batch(3, sizes)


# ------------------------------------------------------------------------------------------------------- the mask mode on the host
@pytest.fixture(scope='module')
def hc():
    return _hostcheck.load('hostcheck_stage_pair')


@pytest.fixture(scope='module')
def pool():
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    images, labels = sc.make_pool_arrays()
    return ResidentPool(ArraySource(images, labels), range(len(images)), 'cpu'), images


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def run_host(hc, pool, index, params, crop):
    """The stage_pair launch on the host: rows `params` (k, 24) over the entries `index`, no teacher output."""
    k, (H, W) = len(index), crop
    table = np.ascontiguousarray(pool.table)
    idx = pool.entries_of(index)
    p = np.ascontiguousarray(params, dtype=np.float32)
    mean, std = sc.MEAN.astype(np.float32), sc.STD.astype(np.float32)
    image = np.zeros((k, 3, H, W), dtype=np.float32)
    mask = np.full((k, H, W), -1.0, dtype=np.float32)
    hc.hc_pair_stage_batch(_ptr(pool.image_buffer.numpy()), _ptr(table), len(table), _ptr(idx), k, H, W, _ptr(p), _ptr(mean),
                           _ptr(std), None, _ptr(image), _ptr(mask))
    return image, mask


@pytest.mark.parametrize('name', ['hung_flips', 'hung_nonuniform', 'plain_crop', 'rot30_scale1.5_unsup'])
def test_mask_mode_on_the_host(hc, pool, name):
    """Slot 23 = 1 on the rows of the single-view configurations of _stage_cases (entries of 5 x 3 and 1 x 1 pixels, sources smaller
    than the window): the mask is exactly {0, 1} and is the oracle's nearest in-bounds test; the image does not depend on the
    mode, and mode 0 gives the in-bounds weight as before."""
    rp, images = pool
    aug, crop, _, cfg = sc.make_augmenter(name)
    params = aug.draw_params(len(sc.INDEX), rp.sizes_of(sc.INDEX), with_labels=False)
    assert not params[:, 23].any()
    nearest = params.copy()
    nearest[:, 23] = 1.0
    image0, mask0 = run_host(hc, rp, sc.INDEX, params, crop)
    image1, mask1 = run_host(hc, rp, sc.INDEX, nearest, crop)
    assert np.array_equal(image0, image1)
    assert set(np.unique(mask1).tolist()) == {0.0, 1.0}
    fractional = 0
    for i, e in enumerate(sc.INDEX):
        want_img, _, want_lin = pc.oracle_view(images[e], params[i], crop, sc.MEAN, sc.STD)
        _, _, want_near = pc.oracle_view(images[e], nearest[i], crop, sc.MEAN, sc.STD)
        near = sc.near_rounding_boundary(params[i], crop)
        keep = np.ones(crop, dtype=bool) if near is None else ~near
        np.testing.assert_allclose(image0[i][:, keep], want_img[:, keep], rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(mask0[i][keep], want_lin[keep], rtol=1e-5, atol=1e-5)
        assert np.array_equal(mask1[i][keep], want_near[keep]), 'sample {}'.format(i)
        fractional += int(((want_lin > 1e-3) & (want_lin < 1 - 1e-3)).sum())
    if name.startswith('hung'):
        assert fractional > 0                                    # the two modes differ somewhere: the linear mask has edges


def test_pair_rows_on_the_host_vs_oracle(hc, pool):
    """A Hung batch of pairs over the ragged pool through the 2n-row layout of stage_pair: both halves against the oracle."""
    from cutmix_semisup_seg_amd import aug_pairs
    rp, images = pool
    crop, cfg, _, seed, _ = pc.RAGGED['hung']
    n = len(sc.INDEX)
    _, _, infos = pc.make_geometry(crop, cfg, seed).draw_batch(n, rp.sizes_of(sc.INDEX))
    params = np.stack([aug_pairs.pair_rows(info, crop) for info in infos], axis=1)
    pc.assert_pair_branches_covered(cfg, params, crop)
    image, mask = run_host(hc, rp, list(sc.INDEX) * 2, params.reshape(2 * n, 24), crop)
    for v in range(2):
        for i, e in enumerate(sc.INDEX):
            want_img, _, want_mask = pc.oracle_view(images[e], params[v, i], crop, sc.MEAN, sc.STD)
            np.testing.assert_allclose(image[v * n + i], want_img, rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(mask[v * n + i], want_mask, rtol=1e-5, atol=1e-5)
    assert set(np.unique(mask[n:]).tolist()) == {0.0, 1.0}


# ------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture()
def fabricated_tree(tmp_path, monkeypatch):
    tree = load_golden_json('pascal_source')['tree']
    train, val = tree['train'][:8], tree['val'][:4]
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), {k: tree['sizes'][k] for k in train + val}, train, val)
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    return tmp_path


def _assert_refused(trainer_name, args, tmp_path):
    from click.testing import CliRunner
    from cutmix_semisup_seg_amd import job_helper
    trainer = __import__(trainer_name)
    args = ['--job_desc', 'refused'] + args
    # the job function itself raises JobNotRun, before it needs its submit configuration or a GPU ...
    params = {k: v for k, v in trainer.experiment.make_context('experiment', list(args)).params.items() if k != 'job_desc'}
    with pytest.raises(job_helper.JobNotRun, match='run with --synthetic'):
        getattr(trainer, trainer_name)(None, **params)
    # ... which through the command line is a non-zero exit that leaves no log
    res = CliRunner().invoke(trainer.experiment, args)
    assert res.exit_code != 0 and 'run with --synthetic' in res.output + str(res.exception)
    assert not os.path.exists(tmp_path / 'results' / trainer_name / 'log_refused.txt')


@pytest.mark.parametrize('trainer_name', TRAINERS)
def test_no_crop_size_is_refused(trainer_name, fabricated_tree):
    _assert_refused(trainer_name, ['--dataset', 'pascal', '--crop_size', ''], fabricated_tree)


@pytest.mark.parametrize('trainer_name', TRAINERS)
def test_more_than_one_process_is_refused(trainer_name, fabricated_tree, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    _assert_refused(trainer_name, ['--dataset', 'pascal'], fabricated_tree)


@pytest.mark.parametrize('trainer_name', TRAINERS)
def test_a_data_set_other_than_pascal_is_refused(trainer_name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _assert_refused(trainer_name, ['--dataset', 'cityscapes'], tmp_path)


def test_stand_alone_under_the_host_sanitizers():
    """The checker behind its own main, built with -fsanitize=address,undefined, as a process of its own: it draws its own small
    inputs and ends non-zero on a non-finite result or a sanitizer report."""
    assert subprocess.call([_hostcheck.build('hostcheck_stage_pair', sanitize=True)]) == 0
