"""
Mirror of the reference's datapipe/isic2017_dataset.py: the ISIC 2017 skin lesion segmentation set from a ZIP archive
(`[paths] isic2017` names the file). Members `train/<name>_x.png`, `train/<name>_y.png`, `val/...` as in the Cityscapes archive,
plus `rgb_mean_std.pkl`, a pickled dict with `rgb_mean` and `rgb_std`. Same sample list and hold-out rule as Cityscapes. A label
map is binary: stored values >= 127 are the lesion (class 1), the rest background (class 0); there is no void.

The archive is made by convert_isic.py (cutmix-semisup-seg_amd/convert_isic.py) from the four official downloads: an exact integer
area resize and the image statistics on the device (csrc/resize.hip). The reference's converter resizes with cv2.INTER_AREA; an
archive it wrote is read just the same, and the two may differ by a grey level near a half (nothing here was compared with cv2).
"""
import pickle

import numpy as np

from .. import settings
from . import seg_data
from .cityscapes_dataset import xy_sample_names


def _get_isic2017_path(exists=False):
    return settings.get_data_path(config_name='isic2017', exists=exists)


class ISIC2017DataSource(seg_data.ZipDataSource):
    def __init__(self, n_val, val_rng, trainval_perm):
        super(ISIC2017DataSource, self).__init__(_get_isic2017_path(exists=True))
        self.sample_names = xy_sample_names(self.zip_file.namelist())
        self.x_names = ['{}_x.png'.format(name) for name in self.sample_names]
        self.y_names = ['{}_y.png'.format(name) for name in self.sample_names]
        train_ndx = np.array([i for i, name in enumerate(self.sample_names) if name.startswith('train/')])
        val_ndx = np.array([i for i, name in enumerate(self.sample_names) if name.startswith('val/')])
        self.train_ndx, self.val_ndx, self.test_ndx = seg_data.hold_out_split(train_ndx, val_ndx, n_val, val_rng, trainval_perm)

        self.class_names = ['background', 'lesion']
        self.num_classes = len(self.class_names)
        mean_std = pickle.loads(self._read_file_from_zip_as_bytes('rgb_mean_std.pkl'))
        self.rgb_mean = mean_std['rgb_mean']
        self.rgb_std = mean_std['rgb_std']

    def map_labels(self, y):
        return (y >= 127).astype(np.uint8)

    def get_mean_std(self):
        return self.rgb_mean, self.rgb_std
