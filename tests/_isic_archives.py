"""Test helper beside tests/_zip_archives.py: the four "official" ISIC 2017 downloads in miniature, as convert_isic.py reads them.
JPEG images written with PIL (among them a `_superpixels.jpg` the converter must skip and an upper-case `.JPG` it must take), 0/255
PNG masks beside members it must not read. The sample names, their order and their split are those of _zip_archives.ISIC2017, so the
golden of the ZIP sources (tests/golden/zip_sources.json) describes the converted archive too; the sizes are this file's."""
import io
import os
import zipfile

import numpy as np
from PIL import Image

import _zip_archives as Z

SIZES = [(96, 128), (80, 120), (131, 97)]                      # (H, W), handed out in turn
X_FOLDER = dict(train='ISIC-2017_Training_Data', val='ISIC-2017_Validation_Data')
Y_FOLDER = dict(train='ISIC-2017_Training_Part1_GroundTruth', val='ISIC-2017_Validation_Part1_GroundTruth')
UPPER_CASE = 'ISIC_0000003'                                    # the sample whose image member ends in .JPG


def jpeg_bytes(arr):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, 'JPEG', quality=90)
    return buf.getvalue()


def samples(sizes=None):
    """-> [(split, name, (H, W))] in archive order"""
    sizes = SIZES if sizes is None else sizes
    return [(full.split('/')[0], full.split('/')[1], sizes[k % len(sizes)]) for k, (full, _) in enumerate(Z.ISIC2017)]


def write_official_isic(zips_dir, sizes=None, seed=6, skip_mask_of=None, mask_size_of=None, grey_image_of=None):
    """The four archives under `zips_dir` -> [(sample name 'train/<name>', image member, mask member)] in the converter's order
    (training archive first, each in archive order). `skip_mask_of` leaves one sample without its mask, `mask_size_of` =
    (name, (H, W)) gives one mask another size, `grey_image_of` stores one image as a greyscale JPEG."""
    rng = np.random.RandomState(seed)
    os.makedirs(zips_dir, exist_ok=True)
    listed = []
    for split in ('train', 'val'):
        x_path = os.path.join(zips_dir, X_FOLDER[split] + '.zip')
        y_path = os.path.join(zips_dir, Y_FOLDER[split] + '.zip')
        with zipfile.ZipFile(x_path, 'w') as zx, zipfile.ZipFile(y_path, 'w') as zy:
            zx.writestr(X_FOLDER[split] + '/', '')
            zx.writestr('{}/{}_metadata.csv'.format(X_FOLDER[split], X_FOLDER[split]), 'image_id,age_approximate,sex\n')
            for s, name, (h, w) in samples(sizes):
                if s != split:
                    continue
                x = Z._image(rng, h, w)
                y = (Z._labels(rng, h, w, [0, 1]) * 255).astype(np.uint8)
                x_member = '{}/{}.{}'.format(X_FOLDER[split], name, 'JPG' if name == UPPER_CASE else 'jpg')
                y_member = '{}/{}_segmentation.png'.format(Y_FOLDER[split], name)
                zx.writestr(x_member, jpeg_bytes(x[..., 1] if name == grey_image_of else x))
                if name == 'ISIC_0000011':
                    zx.writestr('{}/{}_superpixels.jpg'.format(X_FOLDER[split], name), jpeg_bytes(Z._image(rng, h, w)))
                zx.writestr('{}/{}_superpixels.png'.format(X_FOLDER[split], name), Z.png_bytes(Z._image(rng, 8, 8)))
                if name != skip_mask_of:
                    if mask_size_of is not None and mask_size_of[0] == name:
                        y = (Z._labels(rng, mask_size_of[1][0], mask_size_of[1][1], [0, 1]) * 255).astype(np.uint8)
                    zy.writestr(y_member, Z.png_bytes(y))
                listed.append(('{}/{}'.format(split, name), x_member, y_member))
    return listed


def decode_members(zips_dir, listed):
    """PIL's own decode of the members -> {sample name: (image uint8 (H, W, 3), mask uint8 (H, W))}"""
    content = {}
    for sample, x_member, y_member in listed:
        split = sample.split('/')[0]
        with zipfile.ZipFile(os.path.join(zips_dir, X_FOLDER[split] + '.zip')) as zx:
            x = np.array(Image.open(io.BytesIO(zx.read(x_member))))
        with zipfile.ZipFile(os.path.join(zips_dir, Y_FOLDER[split] + '.zip')) as zy:
            y = np.array(Image.open(io.BytesIO(zy.read(y_member))))
        content[sample] = (x, y)
    return content
