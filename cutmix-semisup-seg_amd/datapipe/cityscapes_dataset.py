"""
Mirror of the reference's datapipe/cityscapes_dataset.py: Cityscapes from the ZIP archive that convert_cityscapes.py writes
(`[paths] cityscapes` names the file). Members:

    train/<city>/<city>_<seq>_<frame>_x.png    the (downsampled) left 8-bit image
    train/<city>/<city>_<seq>_<frame>_y.png    its gtFine labelIds map, raw ids 0..33
    val/...

`sample_names` are the members `*_x.png` without that suffix, sorted; the `train/` and `val/` prefixes give `train_ndx` and
`val_ndx`; the hold-out rule of `n_val > 0` and the `trainval_perm` re-ordering are the reference's (seg_data.hold_out_split).
The 34 label ids (and license_plate, the 35th name) are mapped to the 19 training classes and 255 = void when a label map is
read, unless `with_void`; the converter stores raw ids.
"""
import os

import numpy as np

from .. import settings
from . import seg_data

CLASS_NAMES_WITH_VOID = [
    'unlabeled', 'ego_vehicle', 'rectification_border', 'out_of_roi', 'static', 'dynamic', 'ground',
    'road', 'sidewalk', 'parking', 'rail_track',
    'building', 'wall', 'fence', 'guard_rail', 'bridge', 'tunnel',
    'pole', 'pole_group', 'traffic_light', 'traffic_sign',
    'vegetation', 'terrain', 'sky',
    'person', 'rider',
    'car', 'truck', 'bus', 'caravan', 'trailer', 'train', 'motorcycle', 'bicycle',
    'license_plate',
]

VOID_CLASS_NAMES = [
    'unlabeled', 'ego_vehicle', 'rectification_border', 'out_of_roi', 'static', 'dynamic', 'ground',
    'parking', 'rail_track',
    'guard_rail', 'bridge', 'tunnel',
    'pole_group',
    'caravan', 'trailer',
    'license_plate',
]

VOID_CLASS_INDICES = np.array([CLASS_NAMES_WITH_VOID.index(name) for name in VOID_CLASS_NAMES])

CLASS_NAMES = [name for name in CLASS_NAMES_WITH_VOID if name not in VOID_CLASS_NAMES]


def _get_cityscapes_path(exists=False):
    return settings.get_data_path(config_name='cityscapes', exists=exists)


def xy_sample_names(namelist):
    """the sorted sample names of an archive whose samples are pairs `<name>_x.png` / `<name>_y.png`"""
    names = set()
    for filename in namelist:
        x_name, ext = os.path.splitext(filename)
        if x_name.endswith('_x') and ext.lower() == '.png':
            names.add(x_name[:-2])
    return sorted(names)


class CityscapesDataSource(seg_data.ZipDataSource):
    def __init__(self, n_val, val_rng, trainval_perm, with_void=False):
        super(CityscapesDataSource, self).__init__(_get_cityscapes_path(exists=True))
        self.sample_names = xy_sample_names(self.zip_file.namelist())
        self.x_names = ['{}_x.png'.format(name) for name in self.sample_names]
        self.y_names = ['{}_y.png'.format(name) for name in self.sample_names]
        train_ndx = np.array([i for i, name in enumerate(self.sample_names) if name.startswith('train/')])
        val_ndx = np.array([i for i, name in enumerate(self.sample_names) if name.startswith('val/')])
        self.train_ndx, self.val_ndx, self.test_ndx = seg_data.hold_out_split(train_ndx, val_ndx, n_val, val_rng, trainval_perm)

        self.class_names_with_void = CLASS_NAMES_WITH_VOID
        self.void_class_names = VOID_CLASS_NAMES
        self.void_class_indices = VOID_CLASS_INDICES
        self.class_names = CLASS_NAMES
        self.with_void = with_void
        # void -> 255, the others renumbered in order
        mapping, out_cls_i = [], 0
        for name in self.class_names_with_void:
            if name in self.void_class_names:
                mapping.append(255)
            else:
                mapping.append(out_cls_i)
                out_cls_i += 1
        self.non_void_mapping = np.array(mapping)
        self.num_classes_with_void = len(self.class_names_with_void)
        self.num_classes = len(self.class_names)

    def map_labels(self, y):
        if self.with_void:
            return y
        if y.size and int(y.max()) >= len(self.non_void_mapping):
            raise ValueError('{}: label id {} is not one of the {} Cityscapes ids'.format(self.zip_path, int(y.max()),
                                                                                         len(self.non_void_mapping)))
        return self.non_void_mapping.astype(np.uint8)[y]
