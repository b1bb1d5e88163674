"""
Mirror of the reference's datapipe/datasets.py `load_dataset`: the data source plus the supervised / unsupervised / validation
/ test index arrays, with the arithmetic of datasets.py:47-86. Pascal VOC (`pascal`, `pascal_aug`) is built; CamVid, Cityscapes
and ISIC 2017 need ZIP readers and load-time resizing that are not.
"""
import pickle

import numpy as np

from .. import job_helper
from . import pascal_voc_dataset

BUILT = ('pascal', 'pascal_aug')
KNOWN = ('camvid', 'cityscapes', 'pascal', 'pascal_aug', 'isic2017')


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


def load_dataset(dataset, n_val, val_seed, n_sup, n_unsup, split_seed, split_path):
    """-> dict(ds_src, ds_tgt, val_ndx_src, val_ndx_tgt, test_ndx_tgt, sup_ndx, unsup_ndx), the reference's keys"""
    if dataset in KNOWN and dataset not in BUILT:
        raise job_helper.JobNotRun('The data set path is built for {} only; `{}` is not (its ZIP readers and load-time resizing '
                                   'are out of scope). Use one of those, or run with --synthetic.'.format(' and '.join(BUILT), dataset))
    if dataset not in BUILT:
        raise ValueError('Unknown dataset {}'.format(dataset))

    trainval_perm = None
    if split_path is not None:
        with open(split_path, 'rb') as f:
            trainval_perm = pickle.load(f)
    source = pascal_voc_dataset.PascalVOCDataSource(n_val=n_val, val_rng=np.random.RandomState(val_seed),
                                                    trainval_perm=trainval_perm, augmented=dataset == 'pascal_aug')
    n_train = len(source.train_ndx)
    # a split file has already ordered the training samples inside the source; otherwise the order is drawn from split_seed
    order = np.arange(n_train) if split_path is not None else np.random.RandomState(split_seed).permutation(n_train)
    sup_ndx, unsup_ndx = _take(source.train_ndx, order, n_sup, n_unsup)
    return dict(ds_src=source, ds_tgt=source, val_ndx_src=source.val_ndx, val_ndx_tgt=source.val_ndx,
                test_ndx_tgt=source.test_ndx, sup_ndx=sup_ndx, unsup_ndx=unsup_ndx)
