"""Test helper: writes fabricated CamVid, Cityscapes and ISIC 2017 archives in the layout the reference's ZIP data sources read, the
two "official" Cityscapes downloads the converter reads, and the `semantic_segmentation.cfg` that points at them. Content is
seeded noise: the same call writes the same pixels, so the golden generator (tests/golden/make_zip_sources_golden.py) and the
tests rebuild identical archives. Members are written in a deliberately unsorted order, beside members the sources must ignore."""
import io
import os
import pickle
import zipfile

import numpy as np
from PIL import Image

# (sample name, (H, W)): two cities per split, not in sorted order
CITYSCAPES = [('train/zurich/zurich_000002_000019', (72, 96)), ('val/munster/munster_000001_000019', (80, 88)),
              ('train/aachen/aachen_000010_000019', (70, 100)), ('train/zurich/zurich_000000_000019', (76, 92)),
              ('val/frankfurt/frankfurt_000000_000294', (72, 96)), ('train/aachen/aachen_000003_000019', (84, 80)),
              ('train/aachen/aachen_000000_000019', (72, 96)), ('val/frankfurt/frankfurt_000001_000019', (90, 72)),
              ('train/zurich/zurich_000001_000019', (72, 104)), ('train/aachen/aachen_000002_000019', (78, 86)),
              ('val/munster/munster_000000_000019', (72, 96)), ('train/zurich/zurich_000003_000019', (88, 74))]
ISIC2017 = [('train/ISIC_0000011', (70, 94)), ('val/ISIC_0001769', (82, 76)), ('train/ISIC_0000003', (96, 72)),
            ('train/ISIC_0012086', (74, 90)), ('train/ISIC_0000000', (72, 96)), ('val/ISIC_0012255', (72, 96)),
            ('train/ISIC_0000007', (80, 80)), ('val/ISIC_0001960', (71, 103)), ('train/ISIC_0010459', (86, 78)),
            ('train/ISIC_0000001', (72, 96)), ('val/ISIC_0015155', (90, 70)), ('train/ISIC_0009995', (77, 85))]
# (directory, file name, (H, W))
CAMVID = [('CamVid/train', 'Seq05VD_f00000.png', (72, 96)), ('CamVid/test', '0001TP_008550.png', (72, 96)),
          ('CamVid/train', '0006R0_f00930.png', (80, 90)), ('CamVid/val', '0016E5_08001.png', (72, 96)),
          ('CamVid/train', '0001TP_006690.png', (70, 100)), ('CamVid/test', 'Seq05VD_f05100.png', (88, 74)),
          ('CamVid/val', '0016E5_07959.png', (76, 92)), ('CamVid/train', '0016E5_00390.png', (72, 96)),
          ('CamVid/train', '0006R0_f02400.png', (84, 82)), ('CamVid/test', '0001TP_007500.png', (75, 91)),
          ('CamVid/val', '0016E5_08159.png', (90, 72)), ('CamVid/train', '0016E5_01230.png', (72, 104))]
ISIC_MEAN_STD = dict(rgb_mean=np.array([0.708, 0.582, 0.536]), rgb_std=np.array([0.098, 0.113, 0.128]))
# the order in which a split file hands out the training samples (8 train members in Cityscapes and ISIC 2017; CamVid ignores it)
PERM = [5, 2, 7, 0, 3, 6, 1, 4]
VAL_SEED = 131


def png_bytes(arr, bits=8):
    """uint8 (H, W, 3) -> RGB PNG; (H, W) -> greyscale PNG of 8 or 16 bits"""
    buf = io.BytesIO()
    if arr.ndim == 2 and bits == 16:
        Image.fromarray(arr.astype(np.uint16)).save(buf, 'PNG')
    else:
        Image.fromarray(arr.astype(np.uint8)).save(buf, 'PNG')
    return buf.getvalue()


def _image(rng, h, w):
    """smooth-ish noise: 4 x 4 blocks keep the files small"""
    return rng.randint(0, 256, size=(h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(np.uint8)


def _labels(rng, h, w, values):
    """8 x 8 blocks of values drawn from `values`, then 20 % of the pixels redrawn one by one; every value occurs"""
    values = np.asarray(values)
    lab = values[rng.randint(0, len(values), size=(h // 8 + 1, w // 8 + 1))].repeat(8, 0).repeat(8, 1)[:h, :w]
    redraw = rng.uniform(size=(h, w)) < 0.2
    lab = np.where(redraw, values[rng.randint(0, len(values), size=(h, w))], lab)
    lab.reshape(-1)[:len(values)] = values
    return lab.astype(np.int64)


def write_cityscapes(path, seed=1):
    """raw ids 0..33; every second label member is a 16-bit PNG, the others 8-bit -> {sample name: (image, raw labels)}"""
    rng = np.random.RandomState(seed)
    content = {}
    with zipfile.ZipFile(path, 'w') as z:
        z.writestr('README.txt', 'fabricated')
        for k, (name, (h, w)) in enumerate(CITYSCAPES):
            x, y = _image(rng, h, w), _labels(rng, h, w, np.arange(34))
            z.writestr(name + '_y.png', png_bytes(y, bits=16 if k % 2 else 8))
            z.writestr(name + '_x.png', png_bytes(x))
            content[name] = (x, y.astype(np.uint8))
        z.writestr('train/aachen/notes_x.txt', 'not a sample')
    return content


def write_isic2017(path, seed=2):
    """label values straddle the threshold: 0, 126, 127, 128, 255 -> {sample name: (image, stored labels)}"""
    rng = np.random.RandomState(seed)
    content = {}
    with zipfile.ZipFile(path, 'w') as z:
        for name, (h, w) in ISIC2017:
            x, y = _image(rng, h, w), _labels(rng, h, w, [0, 126, 127, 128, 255])
            z.writestr(name + '_x.png', png_bytes(x))
            z.writestr(name + '_y.png', png_bytes(y))
            content[name] = (x, y.astype(np.uint8))
        z.writestr('rgb_mean_std.pkl', pickle.dumps(ISIC_MEAN_STD))
    return content


def write_camvid(path, seed=3):
    """labels 0..11 (11 = void) -> {file name: (image, stored labels)}"""
    rng = np.random.RandomState(seed)
    content = {}
    with zipfile.ZipFile(path, 'w') as z:
        z.writestr('CamVid/train.txt', 'a list the source does not read')
        for dir_name, name, (h, w) in CAMVID:
            x, y = _image(rng, h, w), _labels(rng, h, w, np.arange(12))
            z.writestr(dir_name + 'annot/' + name, png_bytes(y))
            z.writestr(dir_name + '/' + name, png_bytes(x))
            content[name] = (x, y.astype(np.uint8))
    return content


def write_config(cwd, **paths):
    """./semantic_segmentation.cfg with the given [paths] keys"""
    with open(os.path.join(cwd, 'semantic_segmentation.cfg'), 'w') as f:
        f.write('[paths]\n' + ''.join('{}={}\n'.format(k, v) for k, v in paths.items()))


def write_all(cwd):
    """the three archives under `cwd` and the configuration that names them -> {data set: content}"""
    content = dict(cityscapes=write_cityscapes(os.path.join(cwd, 'cityscapes.zip')),
                   isic2017=write_isic2017(os.path.join(cwd, 'isic2017.zip')),
                   camvid=write_camvid(os.path.join(cwd, 'CamVidData.zip')))
    write_config(cwd, cityscapes=os.path.join(cwd, 'cityscapes.zip'), isic2017=os.path.join(cwd, 'isic2017.zip'),
                 camvid=os.path.join(cwd, 'CamVidData.zip'))
    return content


def write_official_cityscapes(left_path, gt_path, names=None, size=(32, 64), seed=4, compress=False):
    """The two official downloads in miniature: leftImg8bit/<split>/<city>/<sample>_leftImg8bit.png (with a test split the
    converter must skip) and gtFine/.../<sample>_gtFine_labelIds.png beside the colour and instance maps it must not read.
    -> {sample name: (image, raw labels)} of the train and val samples"""
    rng = np.random.RandomState(seed)
    names = [n for n, _ in CITYSCAPES] if names is None else names
    h, w = size
    mode = zipfile.ZIP_DEFLATED if compress else zipfile.ZIP_STORED
    content = {}
    with zipfile.ZipFile(left_path, 'w', mode) as zx, zipfile.ZipFile(gt_path, 'w', mode) as zy:
        zx.writestr('README', 'fabricated')
        zx.writestr('leftImg8bit/test/berlin/berlin_000000_000019_leftImg8bit.png', png_bytes(_image(rng, h, w)))
        for name in names:
            x = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
            y = _labels(rng, h, w, np.arange(34)).astype(np.uint8)
            zx.writestr('leftImg8bit/{}_leftImg8bit.png'.format(name), png_bytes(x))
            zy.writestr('gtFine/{}_gtFine_labelIds.png'.format(name), png_bytes(y))
            zy.writestr('gtFine/{}_gtFine_color.png'.format(name), png_bytes(_image(rng, h, w)))
            content[name] = (x, y)
    return content
