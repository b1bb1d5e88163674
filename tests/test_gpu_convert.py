"""
GPU: the converter's downsampling kernels (csrc/convert.hip through ops.downsample_image_u8 / downsample_labels_u8) bit for bit
against the numpy restatement of the reference's arithmetic (tests/_convert_refs.py), with the output poisoned beforehand and
guard bytes behind it; then end to end through the command lines: the converter on fabricated "official" archives, the archive it
writes read back by CityscapesDataSource, and the four trainers on Cityscapes, CamVid and ISIC 2017 archives
(tests/_zip_archives.py) with the index counts tests/golden/zip_sources.json implies.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden_json
import _convert_refs as R
import _zip_archives as Z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = load_golden_json('zip_sources')
GUARD = 64
POISON = 0xA5


def run_op(x, d, misalign=0):
    """x uint8 (N,H,W,3) or (N,H,W) -> the op's output as numpy. The output lives inside a poisoned buffer with GUARD bytes on
    either side, which must come back untouched; `misalign` shifts source and destination off their 4-byte alignment."""
    from cutmix_semisup_seg_amd import ops
    x = np.ascontiguousarray(x, dtype=np.uint8)
    op = ops.downsample_image_u8 if x.ndim == 4 else ops.downsample_labels_u8
    n, h, w = x.shape[:3]
    shape = (n, h // d, w // d) + ((3,) if x.ndim == 4 else ())
    n_out = int(np.prod(shape))
    src_buf = torch.zeros(x.size + 4, dtype=torch.uint8, device=DEV)
    src = src_buf[misalign:misalign + x.size].view(x.shape)
    src.copy_(torch.from_numpy(x))
    buf = torch.full((GUARD + n_out + GUARD + 4,), POISON, dtype=torch.uint8, device=DEV)
    lo = GUARD + misalign
    out = buf[lo:lo + n_out].view(shape)
    assert src.data_ptr() % 4 == misalign and out.data_ptr() % 4 == misalign and src.is_contiguous() and out.is_contiguous()
    got = op(src, d, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:lo] == POISON).all() and (host[lo + n_out:] == POISON).all(), 'a store outside the output'
    return host[lo:lo + n_out].reshape(shape)


IMAGE_SHAPES = [(1, 2, 2, 2), (1, 3, 3, 3), (2, 8, 8, 8), (1, 6, 390, 2), (3, 14, 518, 7), (1, 5, 7, 1),
                # beyond the issue's list: whole groups on the word path (pitch and base on 4 bytes), more than one workgroup
                (2, 4, 32, 2), (2, 16, 520, 4), (1, 10, 45, 5), (1, 12, 54, 6), (1, 9, 48, 3)]


@pytest.mark.parametrize('shape', IMAGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_image_downsampling_vs_numpy(shape):
    n, h, w, d = shape
    rng = np.random.RandomState(sum(shape))
    noise = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    if d > 1:
        sums = noise.reshape(n, h // d, d, w // d, d, 3).astype(np.int64).sum(axis=(2, 4))
        assert (sums % (d * d) != 0).mean() >= 0.5                   # truncation is exercised: 3/4 of random sums at d = 2
    edge, base = R.floor_not_round_image(rng, n, h, w, d)
    inputs = dict(noise=noise, white=np.full((n, h, w, 3), 255, dtype=np.uint8),
                  channels=np.ascontiguousarray(np.broadcast_to(np.array([11, 130, 251], dtype=np.uint8), (n, h, w, 3))), edge=edge)
    for name, x in inputs.items():
        want = R.block_mean_u8(x, d)
        for misalign in (0, 1):
            got = run_op(x, d, misalign)
            assert np.array_equal(got, want), (name, misalign)
    assert np.array_equal(R.block_mean_u8(edge, d), base)
    assert (R.block_mean_u8(inputs['channels'], d) == np.array([11, 130, 251])).all()


LABEL_SHAPES = [(1, 2, 2, 2), (2, 6, 390, 2), (2, 4, 32, 2), (1, 3, 3, 3), (3, 14, 518, 7), (2, 8, 8, 8), (1, 5, 7, 1), (1, 16, 40, 8),
                (2, 8, 44, 4), (1, 10, 45, 5), (1, 12, 54, 6), (1, 9, 48, 3)]


@pytest.mark.parametrize('shape', LABEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_downsampling_vs_numpy(shape):
    n, h, w, d = shape
    rng = np.random.RandomState(sum(shape) + 1)
    for hi in (34, 256):                                              # the Cityscapes ids; every byte value
        y = rng.randint(0, hi, size=(n, h, w)).astype(np.uint8)
        want = R.block_vote(y, d)
        for misalign in (0, 3):
            assert np.array_equal(run_op(y, d, misalign), want), (hi, misalign)


def test_label_vote_ties():
    rng = np.random.RandomState(5)
    two = rng.randint(0, 2, size=(2, 32, 66)).astype(np.uint8)
    want = R.block_vote(two, 2)
    ties = (two.reshape(2, 16, 2, 33, 2).sum(axis=(2, 4)) == 2)
    assert ties.mean() >= 0.25                                        # 6/16 of random blocks are 2-2 ties
    assert (want[ties] == 0).all()                                    # ... which the lower value wins
    assert np.array_equal(run_op(two, 2), want)
    y, winners = R.hand_made_ties()
    assert np.array_equal(R.block_vote(y, 2), winners) and np.array_equal(run_op(y, 2), winners)
    distinct, lowest = R.distinct_blocks(rng)
    assert np.array_equal(R.block_vote(distinct, 8), lowest) and np.array_equal(run_op(distinct, 8), lowest)


def test_full_size_frame_and_the_grid_stride_loop():
    """(1, 1024, 2048) at d = 2, the converter's case, once; and a copy (d = 1) with more work items than the largest grid has
    threads (2048 workgroups of 256), so that the grid-stride loop takes a second turn"""
    rng = np.random.RandomState(9)
    x = rng.randint(0, 256, size=(1, 1024, 2048, 3)).astype(np.uint8)
    assert np.array_equal(run_op(x, 2), R.block_mean_u8(x, 2))
    y = rng.randint(0, 34, size=(1, 1024, 2048)).astype(np.uint8)
    assert np.array_equal(run_op(y, 2), R.block_vote(y, 2))
    y = rng.randint(0, 256, size=(1, 1032, 2048)).astype(np.uint8)
    assert 1032 * 2048 // 4 > 2048 * 256
    assert np.array_equal(run_op(y, 1), y)


def test_results_repeat_and_bad_requests_are_value_errors():
    from cutmix_semisup_seg_amd import ops
    rng = np.random.RandomState(2)
    x = torch.from_numpy(rng.randint(0, 256, size=(2, 12, 36, 3)).astype(np.uint8)).to(DEV)
    assert torch.equal(ops.downsample_image_u8(x, 2), ops.downsample_image_u8(x, 2))
    assert torch.equal(ops.downsample_image_u8(x, 1), x)
    assert torch.equal(ops.downsample_image_u8(x.transpose(1, 2), 3), ops.downsample_image_u8(x.transpose(1, 2).contiguous(), 3))
    with pytest.raises(ValueError):
        ops.downsample_image_u8(x, 5)
    with pytest.raises(ValueError):
        ops.downsample_image_u8(x, 0)
    with pytest.raises(ValueError):
        ops.downsample_labels_u8(x[..., 0].contiguous(), 9)
    with pytest.raises(TypeError):
        ops.downsample_labels_u8(x, 2)
    with pytest.raises(TypeError):
        ops.downsample_image_u8(x, 2, out=torch.empty(2, 6, 18, 3, dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------------------------ end to end
def _convert(cwd, size, d):
    """fabricated official archives of `size` -> the converter's command line -> (path of the archive it wrote, their content)"""
    from click.testing import CliRunner
    import convert_cityscapes as prog
    left, gt = os.path.join(cwd, 'leftImg8bit_trainvaltest.zip'), os.path.join(cwd, 'gtFine_trainvaltest.zip')
    content = Z.write_official_cityscapes(left, gt, size=size, compress=True)
    out = os.path.join(cwd, 'data', 'cityscapes', 'cityscapes_segmentation.zip')
    Z.write_config(cwd, cityscapes=out, camvid=os.path.join(cwd, 'CamVidData.zip'), isic2017=os.path.join(cwd, 'isic2017.zip'))
    res = CliRunner().invoke(prog.convert, [left, gt, '--downsample', str(d)], catch_exceptions=False)
    assert res.exit_code == 0 and 'Writing data to' in res.output, res.output
    return out, content


@pytest.mark.parametrize('size,d', [((32, 64), 2), ((32, 64), 1)], ids=['d2', 'd1'])
def test_converter_cli_writes_what_the_source_reads_back(tmp_path, monkeypatch, size, d):
    import zipfile
    from cutmix_semisup_seg_amd.datapipe import cityscapes_dataset
    monkeypatch.chdir(tmp_path)
    out, content = _convert(str(tmp_path), size, d)
    names = sorted(content)
    with zipfile.ZipFile(out) as z:
        assert sorted(z.namelist()) == sorted(n + s for n in names for s in ('_x.png', '_y.png'))        # no test split
    raw = cityscapes_dataset.CityscapesDataSource(n_val=0, val_rng=np.random.RandomState(0), trainval_perm=None, with_void=True)
    ds = cityscapes_dataset.CityscapesDataSource(n_val=0, val_rng=np.random.RandomState(0), trainval_perm=None)
    case = [c for c in G['cases'] if c['dataset'] == 'cityscapes' and c['n_val'] == 0 and not c['with_perm']][0]
    assert raw.sample_names == names == case['sample_names']
    assert raw.train_ndx.tolist() == case['train_ndx'] and raw.val_ndx.tolist() == case['val_ndx']
    for i, name in enumerate(names):
        x, y = content[name]
        assert raw.get_image_size(i) == (size[0] // d, size[1] // d)
        assert np.array_equal(raw.get_image_arr(i), R.block_mean_u8(x, d))
        assert np.array_equal(raw.get_labels_arr(i), R.block_vote(y, d))
        assert np.array_equal(ds.get_labels_arr(i), np.array(case['non_void_mapping'])[R.block_vote(y, d)])


def _run_trainer(trainer_name, tmp_path, desc, args):
    from click.testing import CliRunner
    trainer = __import__(trainer_name)
    base = ['--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2', '--crop_size', '65,65', '--n_sup', '4',
            '--num_epochs', '1', '--iters_per_epoch', '2']
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', desc] + base + args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    return open(tmp_path / 'results' / trainer_name / 'log_{}.txt'.format(desc)).read()


def _check_log(log, dataset, n_val, n_sup=4):
    """the four len(...)= lines as the reference's sources imply them (the golden), and a finite validation mIoU"""
    case = [c for c in G['cases'] if c['dataset'] == dataset and c['n_val'] == max(n_val, 0) and not c['with_perm']][0]
    assert 'len(sup_ndx)={}\n'.format(n_sup) in log and 'len(unsup_ndx)={}\n'.format(len(case['train_ndx'])) in log
    assert 'len(val_ndx)={}\n'.format(len(case['val_ndx'])) in log
    if case['test_ndx'] is None:
        assert 'len(test_ndx)' not in log and 'FINAL TEST' not in log
    else:
        assert 'len(test_ndx)={}\n'.format(len(case['test_ndx'])) in log
        m = re.search(r'FINAL TEST: mIoU=([0-9.]+)%', log)
        assert m and math.isfinite(float(m.group(1)))
    m = re.search(r'Epoch 1: took [0-9.]+s, TRAIN clf loss=([0-9.naif-]+), consistency loss=([0-9.naif-]+), .*VAL mIoU=([0-9.naif-]+)%', log)
    assert m and all(math.isfinite(float(v)) for v in m.groups()), log


def test_cutmix_trainer_cli_on_a_converted_cityscapes_archive(tmp_path, monkeypatch):
    """The archive is the converter's own output, from 144 x 192 sources at d = 2: its 72 x 96 entries leave room for the 65 x 65 crop
    the network is run at everywhere else in the suite."""
    monkeypatch.chdir(tmp_path)
    _convert(str(tmp_path), (144, 192), 2)
    for desc, extra, n_val in (('city', [], 0), ('city_nval', ['--n_val', '2'], 2)):
        log = _run_trainer('train_seg_semisup_mask_mt', tmp_path, desc,
                           ['--dataset', 'cityscapes', '--aug_hflip', '--aug_strong_colour'] + extra)
        _check_log(log, 'cityscapes', n_val)
        assert ('FINAL TEST: mIoU=' in log) == bool(extra)
        per_class = [l for l in log.splitlines() if l.startswith('-- ') and 'img/s' not in l and 'TEST' not in l][0]
        assert len(per_class[3:].split(', ')) == 19                    # one IoU per training class


def test_cutmix_trainer_cli_on_camvid(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    Z.write_all(str(tmp_path))
    log = _run_trainer('train_seg_semisup_mask_mt', tmp_path, 'camvid', ['--dataset', 'camvid', '--aug_hflip', '--aug_strong_colour'])
    _check_log(log, 'camvid', 0)
    assert 'FINAL TEST: mIoU=' in log                                  # CamVid always has its test set


ISIC_ARGS = ['--dataset', 'isic2017', '--bin_fill_holes']


def test_cutmix_trainer_cli_on_isic2017(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    Z.write_all(str(tmp_path))
    log = _run_trainer('train_seg_semisup_mask_mt', tmp_path, 'isic', ISIC_ARGS + [
        '--aug_hflip', '--aug_vflip', '--aug_hvflip', '--aug_rot_mag', '45', '--aug_max_scale', '1.1'])
    _check_log(log, 'isic2017', 0)


@pytest.mark.parametrize('trainer_name', ['train_seg_semisup_ict', 'train_seg_semisup_vat_mt', 'train_seg_semisup_aug_mt'])
def test_the_other_trainers_run_on_isic2017(trainer_name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    Z.write_all(str(tmp_path))
    log = _run_trainer(trainer_name, tmp_path, 'isic', ISIC_ARGS + ['--aug_scale_hung', '--aug_hflip', '--aug_strong_colour'])
    _check_log(log, 'isic2017', 0)
