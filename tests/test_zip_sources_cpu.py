"""
CPU-only: the ZIP data sources (CamVid, Cityscapes, ISIC 2017) against what the reference's own sources give on the same
fabricated archives (tests/golden/zip_sources.json, generator tests/golden/make_zip_sources_golden.py; the archives are rebuilt
here by tests/_zip_archives.py), their decoding from many threads, the label value check, `load_dataset`'s split arithmetic on a
ZIP source and its refusal of a data set whose archive is not configured.
"""
import os
import pickle
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import load_golden_json
import _zip_archives as Z

G = load_golden_json('zip_sources')


@pytest.fixture(scope='module')
def archives(tmp_path_factory):
    d = tmp_path_factory.mktemp('zip_archives')
    return str(d), Z.write_all(str(d))


@pytest.fixture
def in_archives(archives, monkeypatch):
    monkeypatch.chdir(archives[0])
    return archives[1]


def make_source(dataset, n_val=0, with_perm=False, **kw):
    from cutmix_semisup_seg_amd.datapipe import camvid_dataset, cityscapes_dataset, isic2017_dataset
    cls = dict(camvid=camvid_dataset.CamVidDataSource, cityscapes=cityscapes_dataset.CityscapesDataSource,
               isic2017=isic2017_dataset.ISIC2017DataSource)[dataset]
    return cls(n_val=n_val, val_rng=np.random.RandomState(G['val_seed']), trainval_perm=np.array(G['perm']) if with_perm else None,
               **kw)


def test_the_golden_covers_what_it_should():
    assert G['perm'] == Z.PERM and G['val_seed'] == Z.VAL_SEED
    assert {(c['dataset'], c['n_val'], c['with_perm']) for c in G['cases']} == \
        {(d, n, p) for d in ('camvid', 'cityscapes', 'isic2017') for n in (0, 2) for p in (False, True)}
    for c in G['cases']:
        assert len(c['sample_names']) == 12 and c['sample_names'] == sorted(c['sample_names'])
        assert (c['test_ndx'] is None) == (c['dataset'] != 'camvid' and c['n_val'] == 0)
    assert [n for n, _ in Z.CITYSCAPES] != sorted(n for n, _ in Z.CITYSCAPES)         # the archives are not in sorted order
    assert len({n.split('/')[1] for n, _ in Z.CITYSCAPES}) >= 4                        # two cities per split
    assert all(len(G['labels'][d]) == 2 for d in ('camvid', 'cityscapes', 'isic2017'))


@pytest.mark.parametrize('case', G['cases'], ids=lambda c: '{}-nval{}-{}'.format(c['dataset'], c['n_val'], 'perm' if c['with_perm'] else 'rng'))
def test_sources_equal_the_reference_field_for_field(in_archives, case):
    ds = make_source(case['dataset'], case['n_val'], case['with_perm'])
    assert list(ds.sample_names) == case['sample_names'] and len(ds) == 12
    assert ds.train_ndx.tolist() == case['train_ndx'] and ds.val_ndx.tolist() == case['val_ndx']
    assert (None if ds.test_ndx is None else ds.test_ndx.tolist()) == case['test_ndx']
    assert ds.num_classes == case['num_classes']
    mean, std = ds.get_mean_std()
    assert [float(v) for v in mean] == case['mean'] and [float(v) for v in std] == case['std']
    if case['dataset'] == 'cityscapes':
        assert ds.non_void_mapping.tolist() == case['non_void_mapping']
        assert len(ds.class_names_with_void) == 35 and len(ds.void_class_names) == 16 and len(ds.class_names) == 19
        assert sorted(set(case['non_void_mapping'])) == list(range(19)) + [255]
    if case['dataset'] == 'camvid':
        assert len(ds.class_weights) == 12 and ds.class_weights[-1] == 0 and ds.class_names[-1] == 'void' and ds.num_classes_all == 12


@pytest.mark.parametrize('dataset', ['camvid', 'cityscapes', 'isic2017'])
def test_samples_decode_to_what_the_reference_reads(in_archives, dataset):
    ds = make_source(dataset)
    content = in_archives[dataset]
    for rec in G['labels'][dataset]:
        i = rec['index']
        assert ds.sample_names[i] == rec['sample_name']
        y = ds.get_labels_arr(i)
        assert y.dtype == np.uint8 and list(y.shape) == rec['shape'] and y.flags['C_CONTIGUOUS']
        assert np.array_equal(y.reshape(-1), np.array(rec['values']))
    sizes = dict((n, s) for n, s in Z.CITYSCAPES) if dataset == 'cityscapes' else dict((n, s) for n, s in Z.ISIC2017) \
        if dataset == 'isic2017' else dict((n, s) for _, n, s in Z.CAMVID)
    for i, name in enumerate(ds.sample_names):
        x_want, y_stored = content[name]
        assert ds.get_image_size(i) == sizes[name] == x_want.shape[:2]
        x = ds.get_image_arr(i)
        assert x.dtype == np.uint8 and np.array_equal(x, x_want)
        y = ds.get_labels_arr(i)
        if dataset == 'cityscapes':
            mapping = [c for c in G['cases'] if c['dataset'] == 'cityscapes'][0]['non_void_mapping']
            assert np.array_equal(y, np.array(mapping)[y_stored])
            assert set(np.unique(y).tolist()) == set(range(19)) | {255}
        elif dataset == 'isic2017':
            assert np.array_equal(y, (y_stored >= 127).astype(np.uint8)) and set(np.unique(y_stored).tolist()) == {0, 126, 127, 128, 255}
        else:
            assert np.array_equal(y, np.where(y_stored == 11, 255, y_stored)) and set(np.unique(y).tolist()) == set(range(11)) | {255}
    if dataset == 'cityscapes':
        raw = make_source('cityscapes', with_void=True)
        assert all(np.array_equal(raw.get_labels_arr(i), content[n][1]) for i, n in enumerate(raw.sample_names))
        # both kinds of label member are in the archive
        bits = {zipfile.ZipFile(os.path.join(os.getcwd(), 'cityscapes.zip')).read(n)[24] for n in ds.y_names}
        assert bits == {8, 16}


def test_get_image_size_reads_the_header_only(in_archives, monkeypatch):
    from PIL import Image
    ds = make_source('cityscapes')

    def no_decode(*a, **k):
        raise AssertionError('an image was opened')
    monkeypatch.setattr(Image, 'open', no_decode)
    assert [ds.get_image_size(i) for i in range(len(ds))] == [dict(Z.CITYSCAPES)[n] for n in ds.sample_names]


@pytest.mark.parametrize('dataset', ['camvid', 'cityscapes', 'isic2017'])
def test_threaded_decode_equals_serial_decode(in_archives, dataset):
    ds = make_source(dataset)
    order = list(range(len(ds))) * 4

    def load(i):
        return ds.get_image_size(i), ds.get_image_arr(i), ds.get_labels_arr(i)
    serial = [load(i) for i in range(len(ds))]
    with ThreadPoolExecutor(max_workers=8) as ex:
        threaded = list(ex.map(load, order))
    for i, got in zip(order, threaded):
        assert got[0] == serial[i][0] and np.array_equal(got[1], serial[i][1]) and np.array_equal(got[2], serial[i][2])


def test_pool_packs_a_zip_source(in_archives):
    """What the trainers do with a source: the HBM pool's host half, on eight threads' worth of decoding"""
    from cutmix_semisup_seg_amd.resident_pool import ResidentPool
    ds = make_source('isic2017')
    pool = ResidentPool(ds, list(range(len(ds))), 'cpu', chunk_bytes=50000)
    for i, name in enumerate(ds.sample_names):
        assert np.array_equal(pool.image(i), in_archives['isic2017'][name][0])
        assert np.array_equal(pool.labels(i), (in_archives['isic2017'][name][1] >= 127).astype(np.uint8))


def test_a_label_above_255_is_refused_naming_the_member(tmp_path, monkeypatch):
    path = str(tmp_path / 'cityscapes.zip')
    with zipfile.ZipFile(path, 'w') as z:
        for name, top in (('train/a/a_0', 255), ('train/a/a_1', 256)):
            y = np.zeros((4, 6), dtype=np.uint16)
            y[1, 2] = top
            z.writestr(name + '_x.png', Z.png_bytes(np.zeros((4, 6, 3), dtype=np.uint8)))
            z.writestr(name + '_y.png', Z.png_bytes(y, bits=16))
    Z.write_config(str(tmp_path), cityscapes=path)
    monkeypatch.chdir(tmp_path)
    ds = make_source('cityscapes', with_void=True)
    assert ds.get_labels_arr(0)[1, 2] == 255 and ds.get_labels_arr(0).dtype == np.uint8
    with pytest.raises(ValueError, match='train/a/a_1_y.png'):
        ds.get_labels_arr(1)
    with pytest.raises(ValueError, match='Cityscapes ids'):                          # 255 is no Cityscapes id
        make_source('cityscapes').get_labels_arr(0)


@pytest.mark.parametrize('dataset,n_val,n_sup,n_unsup', [('cityscapes', 0, 4, -1), ('cityscapes', 2, 4, 2), ('isic2017', 2, -1, 3),
                                                         ('isic2017', 0, -1, -1), ('camvid', 0, 4, -1), ('camvid', 2, 3, 2)])
def test_load_dataset_split_arithmetic(in_archives, dataset, n_val, n_sup, n_unsup):
    """datasets.py:47-70 of the reference, restated: one permutation of the training list from split_seed, consecutive slices"""
    from cutmix_semisup_seg_amd.datapipe import datasets
    d = datasets.load_dataset(dataset, n_val, G['val_seed'], n_sup, n_unsup, 12345, None)
    case = [c for c in G['cases'] if c['dataset'] == dataset and c['n_val'] == n_val and not c['with_perm']][0]
    src = d['ds_src']
    assert d['ds_tgt'] is src and src.train_ndx.tolist() == case['train_ndx']
    assert d['val_ndx_tgt'].tolist() == case['val_ndx'] == d['val_ndx_src'].tolist()
    assert (None if d['test_ndx_tgt'] is None else d['test_ndx_tgt'].tolist()) == case['test_ndx']
    train = np.array(case['train_ndx'])
    perm = np.random.RandomState(12345).permutation(len(train))
    want_sup = train if n_sup == -1 else train[perm[:n_sup]]
    if n_unsup == -1:
        want_unsup = train if n_sup == -1 else train[perm]
    else:
        want_unsup = train[perm[n_sup:n_sup + n_unsup]] if n_sup != -1 else train[perm[:n_unsup]]
    assert d['sup_ndx'].tolist() == want_sup.tolist() and d['unsup_ndx'].tolist() == want_unsup.tolist()
    assert not set(d['sup_ndx'].tolist()) & set(d['val_ndx_tgt'].tolist())


def test_load_dataset_with_a_split_file(in_archives, tmp_path):
    from cutmix_semisup_seg_amd.datapipe import datasets
    path = str(tmp_path / 'split.pkl')
    with open(path, 'wb') as f:
        pickle.dump(np.array(G['perm']), f)
    for dataset in ('cityscapes', 'isic2017'):
        d = datasets.load_dataset(dataset, 2, G['val_seed'], 4, -1, 12345, path)
        case = [c for c in G['cases'] if c['dataset'] == dataset and c['n_val'] == 2 and c['with_perm']][0]
        assert d['ds_src'].train_ndx.tolist() == case['train_ndx'] and d['val_ndx_tgt'].tolist() == case['val_ndx']
        assert d['sup_ndx'].tolist() == case['train_ndx'][:4] and d['unsup_ndx'].tolist() == case['train_ndx']     # identity order
    from cutmix_semisup_seg_amd.datapipe import cityscapes_dataset
    with pytest.raises(ValueError, match='trainval_perm'):               # a split file made for another training list
        cityscapes_dataset.CityscapesDataSource(n_val=0, val_rng=np.random.RandomState(0), trainval_perm=np.arange(5))


@pytest.mark.parametrize('dataset', ['camvid', 'cityscapes', 'isic2017'])
def test_an_unconfigured_zip_data_set_is_refused_before_anything_else(dataset, tmp_path, monkeypatch):
    from click.testing import CliRunner
    from cutmix_semisup_seg_amd import job_helper
    from cutmix_semisup_seg_amd.datapipe import datasets
    import train_seg_semisup_mask_mt as trainer
    monkeypatch.chdir(tmp_path)
    others = {k: '/somewhere/{}.zip'.format(k) for k in ('camvid', 'cityscapes', 'isic2017') if k != dataset}
    for configured in (False, True):                          # no configuration file; one that names the other data sets only
        if configured:
            Z.write_config(str(tmp_path), pascal_voc='/somewhere/VOC2012', **others)
        with pytest.raises(job_helper.JobNotRun) as e:
            datasets.load_dataset(dataset, -1, 131, -1, -1, 12345, None)
        msg = str(e.value)
        assert '`{}`'.format(dataset) in msg and '[paths]' in msg and 'semantic_segmentation.cfg' in msg
        assert 'pascal and pascal_aug read a directory tree' in msg and 'camvid, cityscapes and isic2017 read a ZIP file' in msg
        assert msg.endswith('or run with --synthetic')
        res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'unconfigured', '--dataset', dataset])
        assert res.exit_code != 0 and 'read a ZIP file' in res.output + str(res.exception)
        assert not os.path.exists(tmp_path / 'results' / 'train_seg_semisup_mask_mt' / 'log_unconfigured.txt')


def test_a_configured_archive_that_does_not_exist_is_a_data_path_error(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from cutmix_semisup_seg_amd import settings
    from cutmix_semisup_seg_amd.datapipe import datasets
    import train_seg_semisup_mask_mt as trainer
    monkeypatch.chdir(tmp_path)
    Z.write_config(str(tmp_path), camvid=str(tmp_path / 'nowhere_a.zip'), cityscapes=str(tmp_path / 'nowhere_b.zip'),
                   isic2017=str(tmp_path / 'nowhere_c.zip'))
    for dataset, word in (('camvid', 'nowhere_a'), ('cityscapes', 'nowhere_b'), ('isic2017', 'nowhere_c')):
        with pytest.raises(settings.DataPathError, match=word):
            datasets.load_dataset(dataset, -1, 131, -1, -1, 12345, None)
        res = CliRunner().invoke(trainer.experiment, ['--job_desc', 'nozip', '--dataset', dataset])
        assert res.exit_code != 0 and word in res.output + str(res.exception) and 'run with --synthetic' in res.output + str(res.exception)


def test_every_data_set_is_built_and_the_patch_distance_program_stays_pascal_only():
    from cutmix_semisup_seg_amd.datapipe import datasets
    assert set(datasets.BUILT) == set(datasets.KNOWN) == {'camvid', 'cityscapes', 'pascal', 'pascal_aug', 'isic2017'}
    assert set(datasets.ZIP_SETS) | set(datasets.TREE_SETS) == set(datasets.BUILT)
    with pytest.raises(ValueError, match='Unknown dataset'):
        datasets.load_dataset('gtav', -1, 131, -1, -1, 12345, None)
