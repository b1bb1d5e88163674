"""
GPU: the patch-distance analysis on the device (csrc/fft.hip, csrc/patchdist.hip, patch_dist.py, intra_inter_class_patch_dist.py).

  FFT          against numpy.fft on complex128 noise; bound 1e-12 * max|reference|: fp64 eps 2.2e-16 times at most 24 butterfly
               stages (two axes of 4096), times a margin of about 100
  exact D2     torch.equal against the int64 brute force (tests/_patch_dist_refs.py); the rounding residual must stay <= 0.01 (a
               condition: exactness breaks at 0.5, numpy's FFT stays below 6e-6 at the full size)
  goldens      the reference's own maps: |d_device^2 - d_golden^2| <= 10 x the reference's own error against the brute force,
               which the golden script measured and stored
  selection    against the stable numpy selection
  end to end   the command line on a fabricated Pascal VOC tree against the numpy restatement of the whole loop
"""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import load_golden
import _patch_dist_refs as R
import _pascal_tree

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
RESIDUAL_BOUND = 0.01


def _pd():
    from cutmix_semisup_seg_amd import patch_dist
    return patch_dist


def _pool(images, labels=None):
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ArraySource
    return ResidentPool(ArraySource(images, labels), range(len(images)), DEV, with_labels=labels is not None)


# ---------------------------------------------------------------------------------------------------------------------- FFT
@pytest.mark.parametrize('shape', [(1, 8, 8), (3, 16, 8), (2, 64, 128), (1, 8, 4096), (1, 4096, 8), (1, 2048, 16)])
def test_fft2_matches_numpy(shape):
    pd = _pd()
    rng = np.random.RandomState(sum(shape))
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex128)
    fwd, inv = np.fft.fft2(x), np.fft.ifft2(x)
    t = torch.from_numpy(x.copy()).to(DEV)
    assert pd.fft2(t) is t                                                # in place
    got_fwd = t.cpu().numpy()
    e_fwd = np.abs(got_fwd - fwd).max()
    back = pd.fft2(t, inverse=True).cpu().numpy()
    e_rt = np.abs(back - x).max()
    e_inv = np.abs(pd.fft2(torch.from_numpy(x.copy()).to(DEV), inverse=True).cpu().numpy() - inv).max()
    print('fft2 {}: forward {:.3e} (of {:.3e})  inverse {:.3e} (of {:.3e})  round trip {:.3e}'.format(
        shape, e_fwd, np.abs(fwd).max(), e_inv, np.abs(inv).max(), e_rt))
    assert e_fwd <= 1e-12 * np.abs(fwd).max()
    assert e_inv <= 1e-12 * np.abs(inv).max()
    assert e_rt <= 1e-12 * np.abs(x).max()


# ----------------------------------------------------------------------------------------------------------------- exact D2
def _rows(centres, img_i=0):
    return np.array([[img_i, 1, y, x, 0] for y, x in centres], dtype=np.int64)


def _check_exact(image, patch_shape, centres, chunk_size=None, source=None):
    """patches cut at `centres` of `source` (default: the image itself) against every position of `image`"""
    pd = _pd()
    source = image if source is None else source
    pool = _pool([image, source])
    patches = pd.PatchSet(pool, _rows(centres, img_i=1), patch_shape, negatives=False)
    want_patches = np.stack([R.cut_patch(source, patch_shape, yx) for yx in centres])
    kw = {} if chunk_size is None else {'chunk_size': chunk_size}
    got = pd.sqr_distance_maps(pool, 0, patches, **kw)
    want = torch.from_numpy(R.brute_d2(image, want_patches))
    res = pd.last_rounding_residual()
    print('D2 image {} patch {} N {}: residual {:.3e}, max D2 {}'.format(image.shape[:2], patch_shape, len(centres), res, int(want.max())))
    assert got.dtype == torch.int64 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    assert res <= RESIDUAL_BOUND
    q2 = (want_patches ** 2).sum(axis=(1, 2, 3))
    assert np.array_equal(patches.q2.cpu().numpy(), q2)
    return got


def test_d2_is_exact_one_patch_and_five_across_a_chunk_boundary():
    rng = np.random.RandomState(0)
    image = rng.randint(0, 256, size=(13, 17, 3)).astype(np.uint8)
    other = rng.randint(0, 256, size=(13, 17, 3)).astype(np.uint8)
    one = _check_exact(image, (5, 5), [(6, 8)])
    assert int(one[0, 6, 8]) == 0                                         # the anchor's own position
    five = [(0, 0), (12, 16), (6, 8), (3, 15), (11, 1)]                   # corners too: cut from the padded entry
    a = _check_exact(image, (5, 5), five, chunk_size=2, source=other)     # chunks 2 + 2 + 1: a pair, a pair, a remainder
    b = _check_exact(image, (5, 5), five, source=other)                   # one chunk: two pairs and a remainder
    assert torch.equal(a, b)


def test_d2_is_exact_for_a_non_square_patch():
    rng = np.random.RandomState(1)
    image = rng.randint(0, 256, size=(13, 17, 3)).astype(np.uint8)
    _check_exact(image, (3, 7), [(2, 3), (10, 12), (6, 6)])
    _check_exact(image, (7, 3), [(2, 3)])


def test_d2_is_exact_when_the_padding_exceeds_the_image():
    rng = np.random.RandomState(2)
    image = rng.randint(0, 256, size=(5, 9, 3)).astype(np.uint8)          # pad 7 >= H = 5: several reflections
    _check_exact(image, (15, 15), [(2, 4), (0, 8), (4, 0)])


def test_d2_is_zero_everywhere_on_a_saturated_image():
    image = np.full((40, 70, 3), 255, dtype=np.uint8)
    got = _check_exact(image, (9, 9), [(20, 35), (0, 0), (39, 69)])
    assert int(got.abs().max()) == 0


def test_d2_is_exact_at_the_largest_magnitudes():
    """p = 225 on a 64 x 64 image of bright pixels: PQ ~ 1e10, FFT 512 x 512. Checked at 256 sampled positions and at the anchor's
    own position, where D2 == 0."""
    pd = _pd()
    rng = np.random.RandomState(3)
    image = rng.randint(200, 256, size=(64, 64, 3)).astype(np.uint8)
    anchor = (31, 40)
    pool = _pool([image])
    patches = pd.PatchSet(pool, _rows([anchor]), (225, 225), negatives=False)
    got = pd.sqr_distance_maps(pool, 0, patches).cpu().numpy()
    res = pd.last_rounding_residual()
    positions = [anchor] + [(int(y), int(x)) for y, x in zip(rng.randint(0, 64, 256), rng.randint(0, 64, 256))]
    want = R.brute_d2(image, R.cut_patch(image, (225, 225), anchor)[None], positions)
    ys, xs = np.array(positions).T
    print('D2 p=225: residual {:.3e}, max D2 {}, Q2 {}'.format(res, int(want.max()), int(patches.q2[0])))
    assert np.array_equal(got[0, ys, xs], want[0])
    assert got[0, anchor[0], anchor[1]] == 0 and want[0, 0] == 0
    assert got.min() >= 0
    assert res <= RESIDUAL_BOUND


def test_residual_above_the_limit_raises():
    pd = _pd()
    bits = torch.tensor([0.3], dtype=torch.float64, device=DEV).view(torch.int64)
    with pytest.raises(ArithmeticError, match='exact'):
        pd._read_residual(bits)
    assert pd.last_rounding_residual() == pytest.approx(0.3)
    with pytest.raises(ArithmeticError):
        pd._read_residual(torch.tensor([float('nan')], dtype=torch.float64, device=DEV).view(torch.int64))


# ------------------------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('name', ['img_a', 'img_b'])
def test_distance_maps_match_the_reference_goldens(name):
    pd = _pd()
    G = load_golden('patch_dist')
    image, patches, maps = G[name], G[name + '_patches'], G[name + '_maps']
    bound = 10.0 * float(G[name + '_ref_err'])
    assert 0 < bound < 1e-10
    got = np.stack(list(pd.sliding_window_distance_to_patches_generator(image, patches)))
    assert got.dtype == np.float64 and got.shape == maps.shape
    err = np.abs(got ** 2 - maps ** 2).max()
    print('{}: |d^2 - golden^2| max {:.3e}, bound {:.3e}'.format(name, err, bound))
    assert err <= bound
    assert got.min() == 0.0                                               # patch 0 is cut from the image: exactly 0, no float noise
    one = pd.sliding_window_distance_to_patch(image, patches[1])
    assert np.array_equal(one, got[1])


# ---------------------------------------------------------------------------------------------------------------- selection
def _select_reference(keys, mask, k):
    out = []
    for n in range(keys.shape[0]):
        idx = R.select_stable(keys[n], mask[n], k)
        out.append(keys[n][idx])
    return out


def _check_select(keys, mask, k):
    pd = _pd()
    got, count = pd.select_k_smallest(torch.from_numpy(keys).to(DEV), torch.from_numpy(mask).to(DEV), k)
    got, count = got.cpu().numpy(), count.cpu().numpy()
    want = _select_reference(keys, mask, k)
    assert got.shape == (keys.shape[0], k)
    for n, w in enumerate(want):
        assert count[n] == len(w) == min(k, int(mask[n].sum())), n
        assert np.array_equal(got[n, :len(w)], w), n
        assert (got[n, len(w):] == pd.KEY_SENTINEL).all()
    return count


def test_select_k_smallest_with_long_tie_runs():
    """2^19 keys per row but only 6 distinct D2 values: the k-th key sits deep inside a run of equal distances, so every pass down
    to the flat-index bits has to narrow it"""
    rng = np.random.RandomState(4)
    M, N, k = 1 << 19, 3, 1000
    d2 = rng.choice(np.array([0, 1, 255, 65025, 3 * 65025 * 81, (1 << 39) - 2], dtype=np.int64), size=(N, M))
    keys = (d2 << 24) | np.arange(M, dtype=np.int64)[None]
    mask = rng.uniform(size=(N, M)) < 0.3
    mask[2] = rng.uniform(size=M) < 0.001                                 # ~500 candidates < k: the row keeps them all
    count = _check_select(keys, mask, k)
    assert count[0] == count[1] == k and 0 < count[2] < k


def test_select_k_smallest_edges():
    rng = np.random.RandomState(5)
    M = 70001                                                             # no multiple of the block, more than one block
    d2 = rng.randint(0, 50, size=(4, M)).astype(np.int64)
    keys = (d2 << 24) | np.arange(M, dtype=np.int64)[None]
    mask = rng.uniform(size=(4, M)) < 0.5
    mask[1] = False                                                       # an empty mask
    mask[2] = False
    mask[2, [5, 69999, 1234]] = True                                      # three candidates
    mask[3] = True
    _check_select(keys, mask, 1)
    count = _check_select(keys, mask, 7)
    assert count.tolist() == [7, 0, 3, 7]
    _check_select(keys[:, :9], mask[:, :9], 20)                           # k larger than the row
    _check_select(keys[1:2], mask[1:2], 3)                                # nothing but an empty mask
    uint8_mask = torch.from_numpy(mask.astype(np.uint8) * 3).to(DEV)      # any non-zero byte marks a candidate
    got, _ = _pd().select_k_smallest(torch.from_numpy(keys).to(DEV), uint8_mask, 7)
    assert np.array_equal(got.cpu().numpy()[0], _select_reference(keys, mask, 7)[0])


def _check_neighbours(images, labels, patch_shape, rows, k, sample_i, **kw):
    pd = _pd()
    pool = _pool(images, labels)
    patches = pd.PatchSet(pool, rows, patch_shape, negatives=False)
    nb = pd.class_neighbours(pool, sample_i, patches, k, **kw)
    assert pd.last_rounding_residual() <= RESIDUAL_BOUND
    anchors = np.stack([R.cut_patch(images[int(r[0])], patch_shape, r[2:4]) for r in rows])
    d2 = R.brute_d2(images[sample_i], anchors)
    lists = nb.lists()
    assert len(lists) == len(rows)
    for n, (intra, inter) in enumerate(lists):
        w_intra, w_inter = R.class_selection(d2[n], labels[sample_i], rows[n][4], k)
        assert np.array_equal(intra, w_intra), n
        assert np.array_equal(inter, w_inter), n
    return lists


def test_class_neighbours_on_a_constant_image_orders_by_flat_index():
    image = np.full((12, 15, 3), 77, dtype=np.uint8)
    lab = (np.arange(12 * 15).reshape(12, 15) % 3).astype(np.uint8)
    rows = np.array([[0, 1, 6, 7, 0], [0, 1, 2, 3, 2], [0, 1, 5, 5, 1]])
    lists = _check_neighbours([image], [lab], (5, 5), rows, 25, 0)
    intra0 = lists[0][0]
    assert (intra0[:, 0] == 0).all() and np.array_equal(intra0[:, 1] * 15 + intra0[:, 2], np.arange(0, 75, 3))


def test_class_neighbours_excludes_void_and_handles_absent_classes():
    rng = np.random.RandomState(6)
    images = [rng.randint(0, 256, size=(21, 18, 3)).astype(np.uint8), rng.randint(0, 256, size=(14, 23, 3)).astype(np.uint8)]
    labels = [rng.randint(0, 4, size=(21, 18)).astype(np.uint8), rng.randint(0, 2, size=(14, 23)).astype(np.uint8)]
    for lab in labels:
        lab[rng.uniform(size=lab.shape) < 0.2] = 255
    # classes 0 ... 3 and 9; image 1 holds only 0, 1 and void: class 3 and class 9 have no intra pixel there
    rows = np.array([[0, 1, 10, 9, 0], [0, 1, 3, 4, 3], [1, 1, 7, 11, 1], [0, 1, 20, 17, 9], [1, 1, 0, 0, 0]])
    for sample_i in (0, 1):
        lists = _check_neighbours(images, labels, (7, 5), rows, 30, sample_i, chunk_size=2)
        for n, (intra, inter) in enumerate(lists):
            lab = labels[sample_i]
            assert (lab[intra[:, 1], intra[:, 2]] == rows[n][4]).all()
            got = lab[inter[:, 1], inter[:, 2]]
            assert (got != rows[n][4]).all() and (got != 255).all()
    assert len(lists[1][0]) == 0 and len(lists[3][0]) == 0 and len(lists[1][1]) == 30        # sample 1: classes 3, 9 absent
    # k larger than the candidates: every one comes back
    many = _check_neighbours(images, labels, (7, 5), rows[:1], 10 ** 4, 1)
    assert len(many[0][0]) == int((labels[1] == 0).sum()) and len(many[0][1]) == int((labels[1] == 1).sum())


# --------------------------------------------------------------------------------------------------------------- end to end
def test_cli_end_to_end_on_a_fabricated_pascal_tree(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import intra_inter_class_patch_dist as prog
    from cutmix_semisup_seg_amd import patch_dist as pd
    from cutmix_semisup_seg_amd.datapipe import datasets
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool

    train = ['2007_{:06d}'.format(i) for i in range(6)]
    val = ['2008_000001']
    hw = [(40, 56), (64, 48), (48, 48), (41, 63), (57, 50), (50, 61), (44, 44)]
    sizes = dict(zip(train + val, hw))
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), sizes, train, val)
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    base = ['--dataset', 'pascal', '--patch_size', '9', '--n_patches', '7', '--n_neighbours', '20']

    def run(name, extra):
        out = str(tmp_path / name)
        res = CliRunner().invoke(prog.intra_inter_class_patch_dist, [out] + base + extra, catch_exceptions=False)
        assert res.exit_code == 0, res.output
        with open(out, 'rb') as f:
            return pickle.load(f)

    choice = str(tmp_path / 'choice.pkl')
    whole = run('whole.pkl', ['--save_choice', choice])
    monkeypatch.setattr(pd, 'DEFAULT_CHUNK', 3)                           # 4 patches as chunks of 3 + 1
    first = run('first.pkl', ['--batch_size', '4', '--batch', '1', '--batch_index_one_based', '--load_choice', choice])
    second = run('second.pkl', ['--batch_size', '4', '--batch', '1'])

    ds = datasets.load_dataset('pascal', n_val=0, val_seed=0, n_sup=-1, n_unsup=-1, split_seed=12345, split_path=None)['ds_src']
    assert len(ds.train_ndx) == 6
    pool = ResidentPool(ds, ds.train_ndx, DEV, with_labels=True)
    images = {int(i): pool.image(i) for i in ds.train_ndx}
    labels = {int(i): pool.labels(i) for i in ds.train_ndx}
    rows = R.choose_anchors(labels.__getitem__, ds.train_ndx, 7, (9, 9), np.random.RandomState(12345))
    assert len(rows) == 7
    with open(choice, 'rb') as f:
        assert np.array_equal(pickle.load(f), rows)
    want = R.class_distances(images, labels, ds.train_ndx, rows, (9, 9), 20)

    keys = [w + '_image_' + s + '_class' + t for w in ('same', 'other') for s in ('intra', 'inter') for t in ('_dists', '_coords')]
    assert sorted(whole.keys()) == sorted(keys + ['anchor_negative_img_dir_y_x_cls', 'boundary_dists'])
    assert np.array_equal(whole['anchor_negative_img_dir_y_x_cls'], rows)
    assert whole['boundary_dists'].dtype == np.float64
    np.testing.assert_allclose(whole['boundary_dists'], want['boundary_dists'], rtol=1e-12, atol=0)
    for key in keys:
        assert len(whole[key]) == 7
        for p in range(7):
            if key.endswith('_coords'):
                assert whole[key][p].shape[1] == 3 and np.array_equal(whole[key][p], want[key][p]), (key, p)
            else:
                assert whole[key][p].dtype == np.float64
                np.testing.assert_allclose(whole[key][p], want[key][p], rtol=1e-12, atol=0, err_msg='{} {}'.format(key, p))
    # every list is full here (6 images of >= 1900 labelled pixels, 21 classes) except where a class is rare in the own image
    assert all(len(d) == 20 for d in whole['other_image_inter_class_dists'])
    # the anchor itself is among its own image's same-class pixels: the nearest one is at distance exactly 0
    for p in range(7):
        assert whole['same_image_intra_class_dists'][p][0] == 0.0

    # the two batches (4 + 3 patches) concatenate to the unbatched run
    assert len(first['boundary_dists']) == 4 and len(second['boundary_dists']) == 3
    assert np.array_equal(np.concatenate([first['anchor_negative_img_dir_y_x_cls'], second['anchor_negative_img_dir_y_x_cls']]), rows)
    assert np.array_equal(np.concatenate([first['boundary_dists'], second['boundary_dists']]), whole['boundary_dists'])
    for key in keys:
        both = first[key] + second[key]
        assert len(both) == 7
        for p in range(7):
            assert np.array_equal(both[p], whole[key][p]), (key, p)
