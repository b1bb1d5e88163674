"""
GPU: the ISIC 2017 converter's kernels (csrc/resize.hip through ops.resize_area_u8 / sum_sumsq_u8) bit for bit against the numpy
restatement (tests/_resize_refs.py), with the output poisoned beforehand and guard bytes around it; then end to end through the
command lines: the converter on fabricated "official" archives (tests/_isic_archives.py) at three --out_size forms, the archive it
writes read back by ISIC2017DataSource, and the CutMix trainer on the converted archive.
"""
import math
import os
import pickle
import re
import zipfile

import numpy as np
import pytest
import torch

from conftest import load_golden_json
import _resize_refs as R
import _isic_archives as A
import _zip_archives as Z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = load_golden_json('zip_sources')
GUARD = 64
POISON = 0xA5


def run_op(x, ho, wo, misalign=0):
    """x uint8 (N,H,W,3) or (N,H,W) -> the op's output as numpy. The output lives inside a poisoned buffer with GUARD bytes on
    either side, which must come back untouched; `misalign` shifts source and destination off their 4-byte alignment."""
    from cutmix_semisup_seg_amd import ops
    x = np.ascontiguousarray(x, dtype=np.uint8)
    shape = (x.shape[0], ho, wo) + ((3,) if x.ndim == 4 else ())
    n_out = int(np.prod(shape))
    src_buf = torch.zeros(x.size + 4, dtype=torch.uint8, device=DEV)
    src = src_buf[misalign:misalign + x.size].view(x.shape)
    src.copy_(torch.from_numpy(x))
    buf = torch.full((GUARD + n_out + GUARD + 4,), POISON, dtype=torch.uint8, device=DEV)
    lo = GUARD + misalign
    out = buf[lo:lo + n_out].view(shape)
    assert src.data_ptr() % 4 == misalign and out.data_ptr() % 4 == misalign and src.is_contiguous() and out.is_contiguous()
    got = ops.resize_area_u8(src, ho, wo, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:lo] == POISON).all() and (host[lo + n_out:] == POISON).all(), 'a store outside the output'
    return host[lo:lo + n_out].reshape(shape)


@pytest.mark.parametrize('case', R.SMALL_CASES, ids=R.case_id)
def test_resize_vs_numpy(case):
    n, h, w, c, ho, wo = case
    inputs = R.case_inputs(case)
    assert set(inputs) >= {'noise', 'white', 'channels' if c == 3 else 'binary'}
    for name, x in inputs.items():
        want = R.case_want(case, name)
        for misalign in (0, 1):
            assert np.array_equal(run_op(x, ho, wo, misalign), want), (name, misalign)
    assert (R.case_want(case, 'white') == 255).all()            # a weight sum that is off shows here
    if c == 3:
        assert (R.case_want(case, 'channels') == np.array([11, 130, 251])).all()
    if (ho, wo) == (h, w):
        assert np.array_equal(R.case_want(case, 'noise'), inputs['noise'])                 # a copy


def test_ties_go_to_the_even_value():
    """2 x 2 blocks [k, k, k + 1, k + 1] at factor 2: every output is an exact half (asserted on the restatement alone), and the
    answer is k + k % 2"""
    rng = np.random.RandomState(4)
    x, k = R.tie_image(rng)
    assert x.shape == (2, 4, 6, 3)
    assert R.is_tie(x, 2, 3).mean() == 1.0
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    want = R.area_resize_u8(x, 2, 3)
    assert np.array_equal(want, k + k % 2)
    for misalign in (0, 1):
        assert np.array_equal(run_op(x, 2, 3, misalign), want)


def test_one_real_size_frame():
    case = R.FRAME_CASE
    got = run_op(R.case_inputs(case)['noise'], case[4], case[5])
    assert np.array_equal(got, R.case_want(case, 'noise'))


def test_numerators_above_two_to_the_32():
    case = R.BIG_NUMERATOR_CASE
    for name in ('bright', 'white'):
        x = R.case_inputs(case)[name]
        assert R.numerators(x, case[4], case[5]).max() > 2 ** 32
        assert np.array_equal(run_op(x, case[4], case[5]), R.case_want(case, name)), name
    assert (R.case_want(case, 'white') == 255).all()


def test_sum_sumsq_vs_numpy():
    from cutmix_semisup_seg_amd import ops
    rng = np.random.RandomState(6)
    inputs = [rng.randint(0, 256, size=(3, 5, 7, 3)), rng.randint(0, 256, size=(2, 248, 248, 3)), rng.randint(0, 256, size=(1, 1, 1)),
              np.full((1, 248, 248, 3), 255)]
    for x in inputs:
        x = x.astype(np.uint8)
        got = ops.sum_sumsq_u8(torch.from_numpy(x).to(DEV))
        assert got.dtype == torch.int64 and tuple(got.shape) == (x.shape[0], 2 * (3 if x.ndim == 4 else 1))
        assert np.array_equal(got.cpu().numpy(), R.sum_sumsq(x))
    off = torch.zeros(3 * 5 * 7 * 3 + 4, dtype=torch.uint8, device=DEV)[1:1 + 315].view(3, 5, 7, 3)          # a misaligned source
    off.copy_(torch.from_numpy(inputs[0].astype(np.uint8)))
    assert np.array_equal(ops.sum_sumsq_u8(off).cpu().numpy(), R.sum_sumsq(inputs[0].astype(np.uint8)))


def test_results_repeat_and_bad_requests_raise():
    from cutmix_semisup_seg_amd import ops
    rng = np.random.RandomState(2)
    x = torch.from_numpy(rng.randint(0, 256, size=(2, 12, 36, 3)).astype(np.uint8)).to(DEV)
    assert torch.equal(ops.resize_area_u8(x, 5, 7), ops.resize_area_u8(x, 5, 7))
    assert torch.equal(ops.sum_sumsq_u8(x), ops.sum_sumsq_u8(x))
    assert torch.equal(ops.resize_area_u8(x, 12, 36), x)
    xt = x.transpose(1, 2)
    assert not xt.is_contiguous()
    assert torch.equal(ops.resize_area_u8(xt, 7, 5), ops.resize_area_u8(xt.contiguous(), 7, 5))
    assert np.array_equal(ops.resize_area_u8(xt, 7, 5).cpu().numpy(), R.area_resize_u8(xt.contiguous().cpu().numpy(), 7, 5))
    assert torch.equal(ops.sum_sumsq_u8(xt), ops.sum_sumsq_u8(x))
    y = x[..., 0]                                                  # (N,H,W), non-contiguous
    assert np.array_equal(ops.resize_area_u8(y, 5, 7).cpu().numpy(), R.area_resize_u8(y.contiguous().cpu().numpy(), 5, 7))
    for ho, wo in ((13, 36), (12, 37), (0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ValueError):
            ops.resize_area_u8(x, ho, wo)
    with pytest.raises(TypeError):
        ops.resize_area_u8(x.float(), 5, 7)
    with pytest.raises(TypeError):
        ops.resize_area_u8(x[..., :2], 5, 7)                        # two channels
    with pytest.raises(TypeError):
        ops.resize_area_u8(x[0, 0], 5, 7)
    with pytest.raises(TypeError):
        ops.resize_area_u8(x, 5, 7, out=torch.empty(2, 5, 7, 3, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError):
        ops.resize_area_u8(x, 5, 7, out=torch.empty(2, 7, 5, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.sum_sumsq_u8(x.float())
    with pytest.raises(ValueError):
        ops.sum_sumsq_u8(x[:0])


# ------------------------------------------------------------------------------------------------------------ end to end
def _convert(cwd, out_size):
    """fabricated official archives -> the converter's command line -> (path of the archive it wrote, PIL's decode of its inputs)"""
    from click.testing import CliRunner
    import convert_isic as prog
    zips = os.path.join(cwd, 'isic_zips')
    listed = A.write_official_isic(zips)
    out = os.path.join(cwd, 'data', 'isic2017', 'isic2017_segmentation.zip')
    Z.write_config(cwd, isic2017=out, camvid=os.path.join(cwd, 'CamVidData.zip'), cityscapes=os.path.join(cwd, 'cityscapes.zip'))
    res = CliRunner().invoke(prog.convert_isic, [zips, '--out_size', out_size], catch_exceptions=False)
    assert res.exit_code == 0 and 'Writing data to' in res.output, res.output
    assert re.search(r'decode [0-9.]+s, device [0-9.]+s, encode and write [0-9.]+s', res.output), res.output
    return out, listed, A.decode_members(zips, listed)


def _target(h, w, out_size):
    """the issue's rule, restated"""
    if out_size == '':
        return h, w
    if ',' in out_size:
        return tuple(int(v) for v in out_size.split(','))
    s = float(int(out_size)) / float(min(h, w))
    return round(h * s), round(w * s)


@pytest.mark.parametrize('out_size', ['72,72', '65', ''], ids=['fixed', 'shorter_side', 'no_resize'])
def test_converter_cli_writes_what_the_source_reads_back(tmp_path, monkeypatch, out_size):
    from cutmix_semisup_seg_amd.datapipe import isic2017_dataset
    monkeypatch.chdir(tmp_path)
    out, listed, decoded = _convert(str(tmp_path), out_size)
    order = [sample for sample, _, _ in listed]
    assert len(order) == 12 and not any('superpixels' in s for s in order)
    assert [m for _, m, _ in listed if m.endswith('.JPG')] == ['ISIC-2017_Training_Data/{}.JPG'.format(A.UPPER_CASE)]
    with zipfile.ZipFile(out) as z:
        assert z.namelist() == [s + e for s in order for e in ('_x.png', '_y.png')] + ['rgb_mean_std.pkl']     # training set first
        mean_std = pickle.loads(z.read('rgb_mean_std.pkl'))
    ds = isic2017_dataset.ISIC2017DataSource(n_val=0, val_rng=np.random.RandomState(0), trainval_perm=None)
    case = [c for c in G['cases'] if c['dataset'] == 'isic2017' and c['n_val'] == 0 and not c['with_perm']][0]
    assert ds.sample_names == sorted(order) == case['sample_names']
    assert ds.train_ndx.tolist() == case['train_ndx'] and ds.val_ndx.tolist() == case['val_ndx']
    if out_size == '65':
        assert {_target(h, w, out_size) for h, w in A.SIZES} == {(65, 87), (65, 98), (88, 65)}         # 97.5 columns -> 98
    train_images = []
    for i, name in enumerate(ds.sample_names):
        x, y = decoded[name]
        assert x.ndim == 3 and y.ndim == 2 and set(np.unique(y)) <= {0, 255}
        ho, wo = _target(x.shape[0], x.shape[1], out_size)
        want_x, want_y = R.area_resize_u8(x[None], ho, wo)[0], R.area_resize_u8(y[None], ho, wo)[0]
        assert ds.get_image_size(i) == (ho, wo)
        assert np.array_equal(ds.get_image_arr(i), want_x)
        assert np.array_equal(ds.get_raw_labels_arr(i), want_y)
        assert np.array_equal(ds.get_labels_arr(i), (want_y >= 127).astype(np.uint8))
        if name.startswith('train/'):
            train_images.append(want_x)
    assert len(train_images) == 8
    ref_mean, ref_std = R.mean_std(train_images)
    for got, ref in ((mean_std['rgb_mean'], ref_mean), (mean_std['rgb_std'], ref_std), (ds.rgb_mean, ref_mean), (ds.rgb_std, ref_std)):
        assert got.dtype == np.float64 and got.shape == (3,)
        assert np.allclose(got, ref, rtol=1e-9, atol=0), (got, ref)


def test_converter_refuses_at_decode(tmp_path, monkeypatch):
    """a greyscale JPEG among the images: its header gives a size, its decode is not 3-channel"""
    from click.testing import CliRunner
    import convert_isic as prog
    monkeypatch.chdir(tmp_path)
    zips = str(tmp_path / 'zips')
    A.write_official_isic(zips, grey_image_of='ISIC_0000007')
    Z.write_config(str(tmp_path), isic2017=str(tmp_path / 'out' / 'isic2017.zip'))
    res = CliRunner().invoke(prog.convert_isic, [zips, '--out_size', '72,72'])
    assert res.exit_code != 0 and isinstance(res.exception, ValueError)
    assert 'ISIC_0000007.jpg' in str(res.exception) and '3-channel' in str(res.exception)


def _run_trainer(trainer_name, tmp_path, desc, args):
    from click.testing import CliRunner
    trainer = __import__(trainer_name)
    base = ['--arch', 'resnet101_deeplab_imagenet', '--freeze_bn', '--batch_size', '2', '--crop_size', '65,65', '--n_sup', '4',
            '--num_epochs', '1', '--iters_per_epoch', '2']
    res = CliRunner().invoke(trainer.experiment, ['--job_desc', desc] + base + args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    return open(tmp_path / 'results' / trainer_name / 'log_{}.txt'.format(desc)).read()


def _check_log(log, dataset, n_val, n_sup=4):
    """the len(...)= lines as the reference's sources imply them (the golden), and a finite validation mIoU"""
    case = [c for c in G['cases'] if c['dataset'] == dataset and c['n_val'] == max(n_val, 0) and not c['with_perm']][0]
    assert 'len(sup_ndx)={}\n'.format(n_sup) in log and 'len(unsup_ndx)={}\n'.format(len(case['train_ndx'])) in log
    assert 'len(val_ndx)={}\n'.format(len(case['val_ndx'])) in log
    assert case['test_ndx'] is None and 'len(test_ndx)' not in log and 'FINAL TEST' not in log
    m = re.search(r'Epoch 1: took [0-9.]+s, TRAIN clf loss=([0-9.naif-]+), consistency loss=([0-9.naif-]+), .*VAL mIoU=([0-9.naif-]+)%', log)
    assert m and all(math.isfinite(float(v)) for v in m.groups()), log


def test_cutmix_trainer_cli_on_a_converted_isic2017_archive(tmp_path, monkeypatch):
    """The archive is the converter's own output at 72 x 72, which leaves room for the 65 x 65 crop."""
    monkeypatch.chdir(tmp_path)
    _convert(str(tmp_path), '72,72')
    log = _run_trainer('train_seg_semisup_mask_mt', tmp_path, 'isic_converted', ['--dataset', 'isic2017', '--bin_fill_holes'])
    _check_log(log, 'isic2017', 0)
