"""Test helper: writes a fabricated Pascal VOC tree (JPEG images, palette PNG label maps that include 255, the ImageSets lists)
and the `semantic_segmentation.cfg` that points at it. The content is seeded noise; names and sizes come from the caller."""
import os

import numpy as np
from PIL import Image


def _palette():
    pal = []
    for i in range(256):
        pal += [(i * 37) % 256, (i * 91) % 256, (i * 53) % 256]
    return pal


def write_tree(root, sizes, train, val, train_aug=None, seed=0):
    """sizes: name -> (H, W). Writes JPEGImages, SegmentationClass[Aug] and ImageSets/Segmentation[Aug] under `root`."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'JPEGImages'))
    label_dirs = ['SegmentationClass'] + (['SegmentationClassAug'] if train_aug is not None else [])
    for d in label_dirs:
        os.makedirs(os.path.join(root, d))
    for name in sorted(sizes):
        h, w = sizes[name]
        # smooth-ish content (JPEG of pure noise is still valid, this just keeps the files small)
        img = (rng.randint(0, 256, size=(h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w]).astype(np.uint8)
        Image.fromarray(img, 'RGB').save(os.path.join(root, 'JPEGImages', name + '.jpg'), quality=90)
        lab = rng.randint(0, 21, size=(h, w)).astype(np.uint8)
        lab[rng.uniform(size=(h, w)) < 0.1] = 255
        lab[0, 0] = 255
        for d in label_dirs:
            png = Image.fromarray(lab, 'P')
            png.putpalette(_palette())
            png.save(os.path.join(root, d, name + '.png'))
    lists = [('Segmentation', 'train.txt', train)] + ([('SegmentationAug', 'train_aug.txt', train_aug)] if train_aug is not None else [])
    for sub, train_file, names in lists:
        d = os.path.join(root, 'ImageSets', sub)
        os.makedirs(d)
        with open(os.path.join(d, train_file), 'w') as f:
            f.write('\n'.join(names) + '\n\n')
        with open(os.path.join(d, 'val.txt'), 'w') as f:
            f.write('\n'.join(val) + '\n')
    return root


def write_config(cwd, root):
    with open(os.path.join(cwd, 'semantic_segmentation.cfg'), 'w') as f:
        f.write('[paths]\npascal_voc={}\n'.format(root))
