"""
CPU: the host side of the data set path -- the Pascal VOC source, `load_dataset`'s splits, the index streams, the evaluation
canvas, the resident pool's packing, the ragged parameter draws and the trainer's refusals.

What the reference itself can compute on a CPU-only machine comes from tests/golden/pascal_source.json, written by the
reference's own PascalVOCDataSource / RepeatSampler + DataLoader / SegCollate (generator: tests/golden/make_pascal_golden.py).
Its datasets.py pulls in cv2 and cannot be imported, so the split arrays are stated here from datasets.py:47-86. Every data set
is fabricated by the test (tests/_pascal_tree.py): JPEG images and palette PNG label maps that include 255.
"""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import load_golden_json
import _pascal_tree

G = load_golden_json('pascal_source')
TREE = G['tree']
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


@pytest.fixture(scope='module')
def voc(tmp_path_factory):
    cwd = tmp_path_factory.mktemp('voc')
    root = _pascal_tree.write_tree(str(cwd / 'VOC2012'), TREE['sizes'], TREE['train'], TREE['val'], TREE['train_aug'])
    _pascal_tree.write_config(str(cwd), root)
    return cwd


@pytest.fixture
def in_voc(voc, monkeypatch):
    monkeypatch.chdir(voc)
    return voc


@pytest.mark.parametrize('case', G['source'], ids=lambda c: 'aug{augmented:d}_nval{n_val}_perm{with_perm:d}'.format(**c))
def test_source_matches_the_reference(in_voc, case):
    from cutmix_semisup_seg_amd.datapipe.pascal_voc_dataset import PascalVOCDataSource
    perm = np.array(TREE['perm']['aug' if case['augmented'] else 'plain']) if case['with_perm'] else None
    ds = PascalVOCDataSource(n_val=case['n_val'], val_rng=np.random.RandomState(TREE['val_seed']), trainval_perm=perm,
                             augmented=case['augmented'])
    assert list(ds.sample_names) == case['sample_names']
    assert ds.train_ndx.tolist() == case['train_ndx']
    assert ds.val_ndx.tolist() == case['val_ndx']
    assert (None if ds.test_ndx is None else ds.test_ndx.tolist()) == case['test_ndx']
    assert ds.num_classes == case['num_classes'] == 21
    mean, std = ds.get_mean_std()
    assert mean.tolist() == case['mean'] and std.tolist() == case['std']


def test_source_decodes_rgb_and_palette_indices(in_voc):
    from cutmix_semisup_seg_amd.datapipe.pascal_voc_dataset import PascalVOCDataSource
    ds = PascalVOCDataSource(n_val=0, val_rng=np.random.RandomState(0), trainval_perm=None, augmented=True)
    for i in (0, 7, len(ds) - 1):
        name = ds.sample_names[i]
        h, w = TREE['sizes'][name]
        img, lab = ds.get_image_arr(i), ds.get_labels_arr(i)
        assert img.dtype == np.uint8 and img.shape == (h, w, 3) and ds.get_image_size(i) == (h, w)
        assert lab.dtype == np.uint8 and lab.shape == (h, w) and lab[0, 0] == 255
        assert set(np.unique(lab).tolist()) <= set(range(21)) | {255}
        assert np.array_equal(img, np.asarray(Image.open(ds.x_paths[i]).convert('RGB')))
        assert np.array_equal(lab, np.asarray(Image.open(ds.semantic_y_paths[i])))


@pytest.mark.parametrize('n_val', [0, 3])
@pytest.mark.parametrize('n_unsup', [-1, 4])
@pytest.mark.parametrize('n_sup', [-1, 4])
@pytest.mark.parametrize('dataset', ['pascal', 'pascal_aug'])
def test_load_dataset_splits(in_voc, dataset, n_sup, n_unsup, n_val):
    """The arithmetic of datapipe/datasets.py:47-86 for ds_tgt is ds_src, stated here."""
    from cutmix_semisup_seg_amd.datapipe import datasets
    from cutmix_semisup_seg_amd.datapipe.pascal_voc_dataset import PascalVOCDataSource
    d = datasets.load_dataset(dataset, n_val, 131, n_sup, n_unsup, 12345, None)
    src = PascalVOCDataSource(n_val=n_val, val_rng=np.random.RandomState(131), trainval_perm=None, augmented=dataset == 'pascal_aug')
    train = src.train_ndx
    perm = np.random.RandomState(12345).permutation(len(train))
    if n_sup != -1:
        want_sup = train[perm[:n_sup]]
        want_unsup = train[perm[n_sup:n_sup + n_unsup]] if n_unsup != -1 else train[perm]
    else:
        want_sup = train
        want_unsup = train[perm[:n_unsup]] if n_unsup != -1 else train
    assert d['sup_ndx'].tolist() == want_sup.tolist() and d['unsup_ndx'].tolist() == want_unsup.tolist()
    assert d['ds_src'] is d['ds_tgt'] and d['ds_src'].train_ndx.tolist() == train.tolist()
    assert d['val_ndx_tgt'].tolist() == src.val_ndx.tolist() and d['val_ndx_src'] is d['val_ndx_tgt']
    assert (None if d['test_ndx_tgt'] is None else d['test_ndx_tgt'].tolist()) == (None if n_val == 0 else src.test_ndx.tolist())
    # disjoint wherever the reference makes them so: training vs validation (vs test with a hold-out set)
    sup, val = set(d['sup_ndx'].tolist()), set(d['val_ndx_tgt'].tolist())
    assert not sup & val and not set(d['unsup_ndx'].tolist()) & val
    if n_val > 0:
        test = set(d['test_ndx_tgt'].tolist())
        assert not sup & test and not val & test and len(val) == n_val
    if n_sup != -1:
        assert len(sup) == n_sup
        if n_unsup != -1:
            assert not sup & set(d['unsup_ndx'].tolist())             # consecutive slices of one permutation
        else:
            assert sup <= set(d['unsup_ndx'].tolist())                # the whole permuted training set


def test_load_dataset_split_path_and_refusals(in_voc, tmp_path):
    from cutmix_semisup_seg_amd.datapipe import datasets
    from cutmix_semisup_seg_amd import job_helper
    perm = np.array(TREE['perm']['plain'])
    path = str(tmp_path / 'split.pkl')
    with open(path, 'wb') as f:
        pickle.dump(perm, f)
    d = datasets.load_dataset('pascal', 3, 131, 4, 4, 12345, path)
    case = [c for c in G['source'] if not c['augmented'] and c['n_val'] == 3 and c['with_perm']][0]
    train = np.array(case['train_ndx'])
    assert d['ds_src'].train_ndx.tolist() == case['train_ndx']
    assert d['sup_ndx'].tolist() == train[:4].tolist() and d['unsup_ndx'].tolist() == train[4:8].tolist()   # identity train_perm
    assert d['val_ndx_tgt'].tolist() == case['val_ndx'] and d['test_ndx_tgt'].tolist() == case['test_ndx']
    for name in ('camvid', 'cityscapes', 'isic2017'):
        with pytest.raises(job_helper.JobNotRun, match='pascal and pascal_aug'):
            datasets.load_dataset(name, -1, 131, -1, -1, 12345, None)


def test_index_stream_is_the_reference_loader_sequence():
    from cutmix_semisup_seg_amd.datapipe import seg_data
    s = G['streams']
    torch.manual_seed(s['seed'])
    stream, _ = seg_data.repeat_stream(s['ndx'], s['batch_size'])
    it = iter(stream)
    got = [next(it) for _ in range(len(s['batches']))]
    assert got == s['batches']
    flat = [i for b in got for i in b]
    n = len(s['ndx'])
    assert len(flat) > 2 * n                                           # crosses two permutation boundaries
    for k in range(len(flat) // n):
        assert sorted(flat[k * n:(k + 1) * n]) == sorted(s['ndx'])     # a chain of whole permutations
    # the trainer's three streams: supervised, and two unsupervised streams over ONE sampler, iterated independently
    torch.manual_seed(s['trio_seed'])
    sup, _ = seg_data.repeat_stream(s['trio_sup_ndx'], s['batch_size'])
    u0, sampler = seg_data.repeat_stream(s['ndx'], s['batch_size'])
    u1 = seg_data.IndexStream(sampler, s['batch_size'])
    its = [iter(sup), iter(u0), iter(u1)]
    assert [[next(i) for i in its] for _ in range(len(s['trio']))] == s['trio']


@pytest.mark.parametrize('case', G['collate'], ids=lambda c: 'block{}_n{}'.format(c['block_size'][0], len(c['sizes'])))
def test_eval_canvas_is_the_reference_collate(case):
    from cutmix_semisup_seg_amd.datapipe import seg_data
    canvas, offsets = seg_data.collate_geometry(case['sizes'], tuple(case['block_size']))
    assert list(canvas) == case['canvas'] and [list(o) for o in offsets] == case['offsets']


def test_collate_cases_cover_both_axes_and_odd_differences():
    sizes = [s for c in G['collate'] for s in [c['sizes']] if len(s) > 1]
    assert any(len({h for h, _ in s}) > 1 and len({w for _, w in s}) > 1 for s in sizes)
    assert any((max(h for h, _ in s) - min(h for h, _ in s)) % 2 == 1 for s in sizes)
    assert any((max(w for _, w in s) - min(w for _, w in s)) % 2 == 1 for s in sizes)
    assert {tuple(c['block_size']) for c in G['collate']} == {(1, 1), (32, 32)}
    assert seg_data_eval_batches() == [[5, 6, 7], [8]]


def seg_data_eval_batches():
    from cutmix_semisup_seg_amd.datapipe import seg_data
    return seg_data.eval_batches(np.array([5, 6, 7, 8]), 3)


def test_pool_packing(in_voc):
    """Host-visible half of the pool (the device copy is tests/test_gpu_stage.py's): 16-byte starts, no overlap, repeats stored
    once, a tiny chunk size so that the upload goes through several staging buffers, contents equal to a direct PIL decode."""
    from cutmix_semisup_seg_amd.datapipe.pascal_voc_dataset import PascalVOCDataSource
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool, ENTRY_DTYPE, decode_threads
    ds = PascalVOCDataSource(n_val=0, val_rng=np.random.RandomState(0), trainval_perm=None, augmented=True)
    want = [9, 2, 2, 17, 0, 9, 5, 11, 18]
    pool = ResidentPool(ds, want, 'cpu', chunk_bytes=40000)
    uniq = [9, 2, 17, 0, 5, 11, 18]
    assert pool.sample_indices == uniq and len(pool) == len(uniq)
    assert pool.entries_of(want).tolist() == [0, 1, 1, 2, 3, 0, 4, 5, 6] and pool.entries_of(want).dtype == np.int32
    t = pool.table
    assert t.dtype == ENTRY_DTYPE and ENTRY_DTYPE.itemsize == 24 and t['img_off'].dtype == np.int64
    assert pool.table_dev.dtype == torch.uint8 and pool.table_dev.numel() == 24 * len(uniq)
    assert np.array_equal(pool.table_dev.numpy().view(ENTRY_DTYPE), t)
    end_i = end_l = 0
    for e, i in enumerate(uniq):
        h, w = TREE['sizes'][ds.sample_names[i]]
        assert (int(t['hs'][e]), int(t['ws'][e])) == (h, w) == pool.sizes_of([i])[0]
        assert t['img_off'][e] % 16 == 0 and t['lab_off'][e] % 16 == 0
        assert t['img_off'][e] >= end_i and t['lab_off'][e] >= end_l and t['img_off'][e] - end_i < 16    # packed, no overlap
        end_i, end_l = int(t['img_off'][e]) + h * w * 3, int(t['lab_off'][e]) + h * w
        assert np.array_equal(pool.image(i), np.asarray(Image.open(ds.x_paths[i]).convert('RGB')))
        assert np.array_equal(pool.labels(i), np.asarray(Image.open(ds.semantic_y_paths[i])))
    assert pool.image_buffer.numel() == end_i and pool.label_buffer.numel() == end_l     # the last entry ends the buffer
    assert 1 <= decode_threads() <= min(16, len(os.sched_getaffinity(0)))
    with pytest.raises(KeyError):
        pool.entries_of([1])


def test_stage_desc_mirrors_the_header():
    """The ctypes mirrors of the new descriptor and of the entry table have the C compiler's layout (tests/test_abi.py's check,
    for the structs this file's feature adds)."""
    import ctypes
    import subprocess
    import _hostcheck
    from cutmix_semisup_seg_amd import _lib
    from cutmix_semisup_seg_amd.resident_pool import ENTRY_DTYPE
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "cutmixseg.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(cms_stage_desc), offsetof(cms_stage_desc, params), offsetof(cms_stage_desc, n),
         offsetof(cms_stage_desc, out_dtype), sizeof(cms_stage_entry), offsetof(cms_stage_entry, lab_off), offsetof(cms_stage_entry, ws));
  return 0;
}'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        got = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, d)]).decode().split()]
    assert got == [ctypes.sizeof(_lib.StageDesc), _lib.StageDesc.params.offset, _lib.StageDesc.n.offset,
                   _lib.StageDesc.out_dtype.offset, ctypes.sizeof(_lib.StageEntry), _lib.StageEntry.lab_off.offset,
                   _lib.StageEntry.ws.offset]
    assert ENTRY_DTYPE.itemsize == got[4] and ENTRY_DTYPE.fields['lab_off'][1] == got[5] and ENTRY_DTYPE.fields['ws'][1] == got[6]
    # argument validation happens before any HIP call
    d = _lib.StageDesc()
    assert _lib.fn['cms_stage_batch'](ctypes.byref(d), None) == -1 and b'NULL' in _lib.fn['cms_last_error']()
    assert _lib.fn['cms_stage_luma'](ctypes.byref(d), None, None) == -1


@pytest.mark.parametrize('case', load_golden_json('draw_params_single_size'), ids=lambda c: '_'.join(sorted(c['cfg'])))
def test_draw_params_with_one_size_is_unchanged(case):
    """tests/golden/draw_params_single_size.json (generator: tests/golden/make_draw_params_golden.py, run on the commit before
    the ragged path): tables recorded from draw_params as it was before it learnt about ragged
    batches (one (Hs, Ws) per batch), for the same seeds."""
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    aug = DeviceAugmenter(case['crop'], MEAN, STD, rng=np.random.RandomState(case['seed']),
                          colour_rng=np.random.RandomState(case['colour_seed']), **case['cfg'])
    got = aug.draw_params(case['n'], tuple(case['src']), with_labels=case['with_labels'])
    assert got.dtype == np.float32 and np.array_equal(got, np.array(case['table'], dtype=np.float32))
    again = DeviceAugmenter(case['crop'], MEAN, STD, rng=np.random.RandomState(case['seed']),
                            colour_rng=np.random.RandomState(case['colour_seed']), **case['cfg'])
    assert np.array_equal(again.draw_params(case['n'], [case['src']] * case['n'], with_labels=case['with_labels']), got)


@pytest.mark.parametrize('cfg', [dict(scale_hung=True, hflip=True, strong_colour=True), dict(rot_mag=30.0, max_scale=1.5),
                                 dict(vflip=True)], ids=['hung_colour', 'warp', 'crop_vflip'])
def test_draw_params_with_a_list_is_sequential(cfg):
    """Row i of a ragged draw is what a single-sample draw with size i gives at that point of the same random stream."""
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    sizes = [(1, 1), (37, 53), (20, 90), (20, 90), (60, 70), (90, 20), (5, 3), (48, 64)]
    mk = lambda: DeviceAugmenter((48, 64), MEAN, STD, rng=np.random.RandomState(5), colour_rng=np.random.RandomState(6), **cfg)
    whole = mk().draw_params(len(sizes), sizes)
    one_by_one = mk()
    rows = np.concatenate([one_by_one.draw_params(1, s) for s in sizes])
    assert np.array_equal(whole, rows)
    assert len({tuple(r[:4]) + tuple(r[16:22]) for r in whole}) > 1
    with pytest.raises(ValueError):
        mk().draw_params(3, sizes)


def test_trainer_without_a_configuration_refuses_and_leaves_no_log(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_mask_mt as trainer
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'nodata', '--dataset', 'pascal'])
    assert res.exit_code != 0
    assert 'pascal_voc' in res.output and 'semantic_segmentation.cfg' in res.output
    assert not os.path.exists(tmp_path / 'results' / 'train_seg_semisup_mask_mt' / 'log_nodata.txt')
    # a configured path that does not exist, and the data sets that are not built
    _pascal_tree.write_config(str(tmp_path), str(tmp_path / 'nowhere'))
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'nodir', '--dataset', 'pascal_aug'])
    assert res.exit_code != 0 and 'nowhere' in res.output
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'camvid', '--dataset', 'camvid'])
    assert res.exit_code != 0 and 'pascal and pascal_aug' in res.output
    assert not [f for f in os.listdir(tmp_path / 'results' / 'train_seg_semisup_mask_mt') if f.startswith('log_')]
