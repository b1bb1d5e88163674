"""
Mirror of the reference's convert_cityscapes.py: builds the Cityscapes archive that datapipe/cityscapes_dataset.py reads from the
two official downloads.

    python convert_cityscapes.py leftImg8bit_trainvaltest.zip gtFine_trainvaltest.zip [--downsample 2]

Every `leftImg8bit/{train,val}/<city>/<sample>_leftImg8bit.png` (the test split is skipped: it has no public labels) and its
`gtFine/.../<sample>_gtFine_labelIds.png` become `<split>/<city>/<sample>_x.png` and `..._y.png` in the ZIP file that
`[paths] cityscapes` of ./semantic_segmentation.cfg names (its directory is created), downsampled by `--downsample` d:

    images   the mean of each d x d block, truncated to uint8                (skimage downscale_local_mean(...).astype(uint8))
    labels   the most frequent raw id of each d x d block, lowest id on ties (one-hot, block sum, argmax)

Both run on the device (ops.downsample_image_u8 / downsample_labels_u8, csrc/convert.hip), on whole chunks of samples: a chunk is
decoded on at most 16 host threads into one staging array, goes to the device and back once, and is encoded on the same threads.
A chunk holds consecutive samples of one size, as many as fit `chunk_bytes` of decoded pixels, so host memory stays bounded.
`--downsample 1` copies.

Refused before the GPU is touched: d outside 1..8, no `cityscapes` path, an image without its label map, a size that d does not
divide (the reference's label reshape fails there), an image and a label map of different sizes.

Deviations from the reference:
  * label members are written as 8-bit greyscale PNGs, not from a uint32 array (mode 'I'; Pillow deprecates saving that mode as
    PNG). The values are the same, and the readers -- the reference's and datapipe/cityscapes_dataset.py -- accept either.
  * scikit-image and tqdm are not needed.
"""
import click

DEFAULT_CHUNK_BYTES = 256 << 20
MAX_DOWNSAMPLE = 8


def sample_name_of(x_member):
    """'leftImg8bit/train/aachen/aachen_000000_000019_leftImg8bit.png' -> 'train/aachen/aachen_000000_000019', with the
    reference's string arithmetic (convert_cityscapes.py:38)"""
    import os
    return os.path.splitext(x_member)[0].replace('_leftImg8bit', '').replace('leftImg8bit/', '')


def members_to_process(x_namelist):
    """-> [(image member, label member, sample name)] in archive order (convert_cityscapes.py:34-39)"""
    import os
    out = []
    for name in x_namelist:
        if os.path.splitext(name)[1].lower() == '.png' and not name.startswith('leftImg8bit/test'):
            sample_name = sample_name_of(name)
            out.append((name, 'gtFine/{}_gtFine_labelIds.png'.format(sample_name), sample_name))
    return out


def plan_chunks(sizes, chunk_bytes):
    """sizes [(H, W)] -> [(first, last)] runs of consecutive samples of one size whose decoded pixels (4 bytes each: image and
    labels) fit chunk_bytes; a run holds at least one sample"""
    chunks, first = [], 0
    while first < len(sizes):
        h, w = sizes[first]
        room = max(1, int(chunk_bytes) // (h * w * 4))
        last = first + 1
        while last < len(sizes) and last - first < room and sizes[last] == sizes[first]:
            last += 1
        chunks.append((first, last))
        first = last
    return chunks


def check_request(downsample, items, x_sizes, y_sizes):
    """The refusals that need the archives' headers only -> None, or raises SystemExit"""
    d = downsample
    for (x_name, y_name, _), xs, ys in zip(items, x_sizes, y_sizes):
        if xs != ys:
            raise SystemExit('{} is {}x{} but its label map {} is {}x{}'.format(x_name, xs[0], xs[1], y_name, ys[0], ys[1]))
        if xs[0] % d or xs[1] % d:
            raise SystemExit('{} is {}x{}: --downsample {} does not divide it (blocks would straddle the edge; the reference '
                             'fails there too)'.format(x_name, xs[0], xs[1], d))


def convert_archives(leftimg8bit_zip_path, gtfine_zip_path, downsample=2, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """The whole conversion -> dict(n_samples, out_path, seconds=dict(decode, device, encode_write)). Raises SystemExit with
    the reason for everything it refuses; the refusals come before the GPU is touched."""
    import io
    import os
    import time
    import zipfile
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    from PIL import Image

    from . import settings
    from .datapipe import cityscapes_dataset, seg_data
    from .resident_pool import decode_threads

    d = int(downsample)
    if d < 1 or d > MAX_DOWNSAMPLE:
        raise SystemExit('--downsample must be in 1..{} (got {})'.format(MAX_DOWNSAMPLE, d))
    try:
        out_path = cityscapes_dataset._get_cityscapes_path(exists=False)
    except settings.DataPathError as e:
        raise SystemExit('{} -- `cityscapes=<path of the .zip to write>` is where the converted archive goes.'.format(e))
    for path in (leftimg8bit_zip_path, gtfine_zip_path):
        if not os.path.isfile(path):
            raise SystemExit('{} does not exist'.format(path))
    # the archives are read as a ZIP data source reads its own: one ZipFile each for all the threads, raw bytes under a lock
    x_zip, y_zip = seg_data.ZipDataSource(leftimg8bit_zip_path), seg_data.ZipDataSource(gtfine_zip_path)
    items = members_to_process(x_zip.zip_file.namelist())
    if not items:
        raise SystemExit('{} holds no leftImg8bit/train or leftImg8bit/val .png members'.format(leftimg8bit_zip_path))
    y_members = set(y_zip.zip_file.namelist())
    for x_name, y_name, _ in items:
        if y_name not in y_members:
            raise SystemExit('{} has no label map: {} is not in {}'.format(x_name, y_name, gtfine_zip_path))

    with ThreadPoolExecutor(max_workers=decode_threads()) as ex:
        x_sizes = list(ex.map(x_zip.member_size, [it[0] for it in items]))
        y_sizes = list(ex.map(y_zip.member_size, [it[1] for it in items]))
        check_request(d, items, x_sizes, y_sizes)

        # nothing above has touched the GPU
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise SystemExit('convert_cityscapes needs a GPU: the downsampling runs on the device only')
        device = torch.device('cuda', torch.cuda.current_device())

        out_dir = os.path.dirname(out_path)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        print('Writing data to {}'.format(out_path))
        seconds = dict(decode=0.0, device=0.0, encode_write=0.0)
        with zipfile.ZipFile(out_path, 'w') as out_zip:
            for first, last in plan_chunks(x_sizes, chunk_bytes):
                k, (h, w) = last - first, x_sizes[first]
                xs = np.empty((k, h, w, 3), dtype=np.uint8)
                ys = np.empty((k, h, w), dtype=np.uint8)

                def decode(i):
                    x_name, y_name, _ = items[first + i]
                    x = np.asarray(x_zip.get_pil_image(x_name).convert('RGB'), dtype=np.uint8)
                    y = seg_data.labels_from_pil(y_zip.get_pil_image(y_name), y_name)
                    if x.shape != (h, w, 3) or y.shape != (h, w):
                        raise ValueError('{}: decodes to {} / {}, its header says {}x{}'.format(x_name, x.shape, y.shape, h, w))
                    xs[i], ys[i] = x, y

                t0 = time.time()
                list(ex.map(decode, range(k)))
                t1 = time.time()
                x_small = ops.downsample_image_u8(torch.from_numpy(xs).to(device), d).cpu().numpy()
                y_small = ops.downsample_labels_u8(torch.from_numpy(ys).to(device), d).cpu().numpy()
                t2 = time.time()

                def encode(i):
                    bufs = []
                    for arr in (x_small[i], y_small[i]):
                        buf = io.BytesIO()
                        Image.fromarray(arr).save(buf, 'PNG')
                        bufs.append(buf.getvalue())
                    return bufs

                for i, (x_png, y_png) in enumerate(ex.map(encode, range(k))):
                    sample_name = items[first + i][2]
                    out_zip.writestr('{}_x.png'.format(sample_name), x_png)
                    out_zip.writestr('{}_y.png'.format(sample_name), y_png)
                t3 = time.time()
                seconds['decode'] += t1 - t0
                seconds['device'] += t2 - t1
                seconds['encode_write'] += t3 - t2
    print('{} samples, downsample {}: decode {:.1f}s, device {:.1f}s, encode and write {:.1f}s'.format(
        len(items), d, seconds['decode'], seconds['device'], seconds['encode_write']))
    return dict(n_samples=len(items), out_path=out_path, seconds=seconds)


@click.command(help='Cityscapes archive for the trainers from the two official downloads; the downsampling runs on the device. '
                    'Deviation from the reference: label members are 8-bit greyscale PNGs (same values).')
@click.argument('leftimg8bit_trainvaltest_zip_path', type=click.Path(readable=True))
@click.argument('gtfine_trainvaltest_zip_path', type=click.Path(readable=True))
@click.option('--downsample', type=int, default=2)
def convert(leftimg8bit_trainvaltest_zip_path, gtfine_trainvaltest_zip_path, downsample):
    convert_archives(leftimg8bit_trainvaltest_zip_path, gtfine_trainvaltest_zip_path, downsample)


if __name__ == '__main__':
    convert()
