"""
Mirror of the reference's datapipe/datasets.py `load_dataset`: the data source plus the supervised / unsupervised / validation
/ test index arrays, with the arithmetic of datasets.py:47-86. All five data sets of the reference are built: Pascal VOC (`pascal`,
`pascal_aug`) reads a directory tree (`[paths] pascal_voc`); CamVid, Cityscapes and ISIC 2017 each read one ZIP archive
(`[paths] camvid`, `cityscapes`, `isic2017`: the path of the file). A ZIP data set whose path is not configured is refused here,
before a source is built, as a job that does not start.
"""
import pickle

import numpy as np

from .. import job_helper, settings
from . import camvid_dataset, cityscapes_dataset, isic2017_dataset, pascal_voc_dataset

TREE_SETS = ('pascal', 'pascal_aug')                    # read a directory tree
ZIP_SETS = ('camvid', 'cityscapes', 'isic2017')         # read one ZIP file; the name is also the key in [paths]
BUILT = ('camvid', 'cityscapes', 'pascal', 'pascal_aug', 'isic2017')
KNOWN = BUILT


def _take(train_ndx, order, n_sup, n_unsup):
    """The supervised / unsupervised subsets of `train_ndx`, given the order in which the training samples are handed out
    (datasets.py:58-70 for one data set serving both roles). A count of -1 means the whole training set in its own order;
    otherwise supervised samples are the first n_sup of `order` and, when both counts are given, unsupervised samples are the
    n_unsup that follow them (disjoint); with n_sup alone the unsupervised set is every training sample, in `order`."""
    sup = train_ndx if n_sup == -1 else train_ndx[order[:n_sup]]
    if n_unsup == -1:
        unsup = train_ndx if n_sup == -1 else train_ndx[order]
    else:
        first = 0 if n_sup == -1 else n_sup
        unsup = train_ndx[order[first:first + n_unsup]]
    return sup, unsup


def _require_zip_path(dataset):
    """A ZIP data set needs `[paths] <dataset>` in the configuration file; without it the job does not start."""
    try:
        settings.get_data_path(config_name=dataset, exists=False)
    except settings.DataPathError:
        raise job_helper.JobNotRun(
            'The data set `{0}` is not configured: no path `{0}` in section [paths] of {1}. {2} read a directory tree '
            '(`pascal_voc=<directory>`) while {3} read a ZIP file (`{0}=<path of the .zip>`). Add that line, or run with '
            '--synthetic'.format(dataset, settings._CONFIG_PATH, ' and '.join(TREE_SETS),
                                 ', '.join(ZIP_SETS[:-1]) + ' and ' + ZIP_SETS[-1]))


def load_dataset(dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path):
    """-> dict(ds_src, ds_tgt, val_ndx_src, val_ndx_tgt, test_ndx_tgt, sup_ndx, unsup_ndx), the reference's keys"""
    if dataset not in BUILT:
        raise ValueError('Unknown dataset {}'.format(dataset))
    if dataset in ZIP_SETS:
        _require_zip_path(dataset)

    trainval_perm = None
    if split_path is not None:
        with open(split_path, 'rb') as f:
            trainval_perm = pickle.load(f)
    val_rng = np.random.RandomState(val_seed)
    if dataset == 'camvid':
        source = camvid_dataset.CamVidDataSource(n_val=n_val, val_rng=val_rng, trainval_perm=trainval_perm)
    elif dataset == 'cityscapes':
        source = cityscapes_dataset.CityscapesDataSource(n_val=n_val, val_rng=val_rng, trainval_perm=trainval_perm)
    elif dataset == 'isic2017':
        source = isic2017_dataset.ISIC2017DataSource(n_val=n_val, val_rng=val_rng, trainval_perm=trainval_perm)
    else:
        source = pascal_voc_dataset.PascalVOCDataSource(n_val=n_val, val_rng=val_rng, trainval_perm=trainval_perm,
                                                        augmented=dataset == 'pascal_aug')
    n_train = len(source.train_ndx)
    # a split file has already ordered the training samples inside the source; otherwise the order is drawn from split_seed
    order = np.arange(n_train) if split_path is not None else np.random.RandomState(split_seed).permutation(n_train)
    sup_ndx, unsup_ndx = _take(source.train_ndx, order, n_sup, n_unsup)
    return dict(ds_src=source, ds_tgt=source, val_ndx_src=source.val_ndx, val_ndx_tgt=source.val_ndx,
                test_ndx_tgt=source.test_ndx, sup_ndx=sup_ndx, unsup_ndx=unsup_ndx)
