"""
Mirror of the reference's datapipe/pascal_voc_dataset.py: the Pascal VOC 2012 data source (optionally with the augmented
label set of Hariharan et al. as distributed by Hung et al.). Directory layout, as in the reference:

    <pascal_voc>/JPEGImages/<name>.jpg
                /SegmentationClass/<name>.png            SegmentationClassAug/ for the augmented set
                /ImageSets/Segmentation/{train,val}.txt  ImageSets/SegmentationAug/{train_aug,val}.txt

`sample_names` (sorted union of both lists), `train_ndx`, `val_ndx`, `test_ndx` come out as pascal_voc_dataset.py:46-105
computes them, including the hold-out rule of `n_val > 0` (the validation list becomes the TEST set, the tail of the permuted
training list becomes the validation set) and the `trainval_perm` re-ordering. `fg_class_subset` is not built.

Samples are decoded with PIL: images to RGB uint8 (H, W, 3), label maps to their palette indices uint8 (H, W), 255 = void.
The accessors of the reference (transform pipelines run by loader workers) have no counterpart: the decoded arrays go into
the HBM-resident pool (resident_pool.py) once and every transform runs on the device.
"""
import os

import numpy as np
from PIL import Image

from .. import settings
from . import seg_data


def _load_names(path):
    """the non-empty lines of a name list"""
    with open(path, 'r') as f:
        return [name for name in (line.strip() for line in f) if name]


def _get_pascal_path(exists=False):
    return settings.get_data_path(config_name='pascal_voc', exists=exists)


class PascalVOCDataSource(seg_data.DataSource):
    def __init__(self, n_val, val_rng, trainval_perm, augmented=False):
        pascal_path = _get_pascal_path(exists=True)
        sets_dir, labels_dir, train_list = ('SegmentationAug', 'SegmentationClassAug', 'train_aug.txt') if augmented else \
            ('Segmentation', 'SegmentationClass', 'train.txt')
        train_names = _load_names(os.path.join(pascal_path, 'ImageSets', sets_dir, train_list))
        val_names = _load_names(os.path.join(pascal_path, 'ImageSets', sets_dir, 'val.txt'))

        self.sample_names = sorted(set(train_names + val_names))
        name_to_index = {name: name_i for name_i, name in enumerate(self.sample_names)}
        self.train_ndx = np.array([name_to_index[name] for name in train_names])
        self.val_ndx = np.array([name_to_index[name] for name in val_names])
        self.semantic_y_paths = [os.path.join(pascal_path, labels_dir, '{}.png'.format(name)) for name in self.sample_names]
        # `trainval_perm` (a split file) re-orders the training list. With a hold-out set (n_val > 0) the official validation
        # list becomes the TEST set and the last n_val training samples, in that order or else in one drawn from val_rng, the
        # validation set (pascal_voc_dataset.py:83-101).
        self.test_ndx = None
        order = None
        if trainval_perm is not None:
            if len(trainval_perm) != len(self.train_ndx):
                raise ValueError('trainval_perm has {} entries, the training list {}'.format(len(trainval_perm),
                                                                                            len(self.train_ndx)))
            order = np.asarray(trainval_perm)
        elif n_val > 0:
            order = val_rng.permutation(len(self.train_ndx))
        if order is not None:
            self.train_ndx = self.train_ndx[order]
        if n_val > 0:
            self.test_ndx = self.val_ndx
            self.train_ndx, self.val_ndx = self.train_ndx[:-n_val], self.train_ndx[-n_val:]

        self.x_paths = [os.path.join(pascal_path, 'JPEGImages', '{}.jpg'.format(name)) for name in self.sample_names]
        self.num_classes = 21
        self.class_map = None

    def __len__(self):
        return len(self.sample_names)

    def get_image_arr(self, sample_i):
        """-> uint8 (H, W, 3) RGB"""
        with Image.open(self.x_paths[sample_i]) as img:
            return np.ascontiguousarray(np.asarray(img.convert('RGB'), dtype=np.uint8))

    def get_labels_arr(self, sample_i):
        """-> uint8 (H, W): the PNG's palette indices, 255 = void"""
        with Image.open(self.semantic_y_paths[sample_i]) as img:
            img.load()
            arr = np.asarray(img)
        if arr.ndim != 2:
            raise ValueError('{}: a palette / greyscale label map is expected, got shape {}'.format(
                self.semantic_y_paths[sample_i], arr.shape))
        return np.ascontiguousarray(arr.astype(np.uint8))

    def get_image_size(self, sample_i):
        """-> (H, W) from the file header, without decoding"""
        with Image.open(self.x_paths[sample_i]) as img:
            w, h = img.size
        return int(h), int(w)
