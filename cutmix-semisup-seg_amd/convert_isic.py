"""
Mirror of the reference's convert_isic.py: builds the ISIC 2017 archive that datapipe/isic2017_dataset.py reads from the four
official downloads in one directory.

    python convert_isic.py ISIC_ZIPS_DIR [--out_size 248,248]

ISIC_ZIPS_DIR holds ISIC-2017_Training_Data.zip, ISIC-2017_Training_Part1_GroundTruth.zip, ISIC-2017_Validation_Data.zip and
ISIC-2017_Validation_Part1_GroundTruth.zip. Every `.jpg` member of a data archive whose stem does not end in `_superpixels`, in
archive order, and its mask `<ground truth folder>/<name>_segmentation.png` become `train/<name>_x.png` and `train/<name>_y.png`
(or `val/...`) in the ZIP file that `[paths] isic2017` of ./semantic_segmentation.cfg names (its directory is created), resized to
`--out_size`: `H,W` for a fixed size, one integer for the length of the shorter side (the size is then
(round(h s), round(w s)) with s = out_size / min(h, w) in float64, halves to even), empty for no resize. `rgb_mean_std.pkl`
holds the per-channel mean and standard deviation of the resized TRAINING images, as float64 arrays of shape (3,).

The resize is an exact area filter on the device (ops.resize_area_u8, csrc/resize.hip): along an axis of L source pixels and Lo
output cells, in units of 1 / Lo pixel, pixel i covers [i Lo, (i + 1) Lo), cell o covers [o L, (o + 1) L) and the weight is the
length of their overlap; the output is sum wy wx p / (h w), rounded to nearest, an exact half to the even value. Integer
arithmetic throughout: the archive is the same on every run. The statistics are exact too: sum p and sum p^2 per image and channel
as int64 on the device (ops.sum_sumsq_u8), added up in Python integers, then mean = S / (255 N) and
std = sqrt(S2 / (255^2 N) - mean^2) in float64 -- the reference's formula.

Samples go through in chunks of consecutive samples whose decoded pixels fit `chunk_bytes`: a chunk is decoded on at most 16 host
threads straight into pinned staging tensors, every run of equally sized samples in it goes to the device and back once, and the
results are PNG-encoded on the same threads. The summary line gives the decode / device / encode-and-write seconds.

Refused before the GPU is touched: a malformed --out_size, no `isic2017` path, a missing input archive, a data archive without
.jpg members, an image without its mask, an image and a mask of different sizes, a target larger than a source along either axis
(the area filter only shrinks; cv2 would switch to another filter there). Refused at decode: a mask that is not a 2-D uint8 array,
an image that is not 3-channel.

Deviations from the reference:
  * cv2.INTER_AREA accumulates in float32 and has separate fast paths for integer factors, whose rounding differs between them; its
    result can differ from the definition above by one grey level near a half. With an integer --out_size cv2 also takes its cell
    size from the scale factor, not from the ratio of the two sizes. Nothing here has been compared with cv2, and no bit-identity
    with it is claimed.
  * cv2, scikit-image and tqdm are not needed.
"""
import click

DEFAULT_CHUNK_BYTES = 1 << 30
# (data archive, ground truth archive, ground truth folder inside it, split) -- the reference's fixed names
ARCHIVES = (('ISIC-2017_Training_Data.zip', 'ISIC-2017_Training_Part1_GroundTruth.zip', 'ISIC-2017_Training_Part1_GroundTruth', 'train'),
            ('ISIC-2017_Validation_Data.zip', 'ISIC-2017_Validation_Part1_GroundTruth.zip', 'ISIC-2017_Validation_Part1_GroundTruth',
             'val'))


def parse_out_size(text):
    """'H,W' -> (H, W); 'S' -> S (the shorter side); '' -> None, with the reference's forms (convert_isic.py:19-29). Raises
    SystemExit for anything else."""
    text = '' if text is None else str(text)
    try:
        if ',' in text:
            h, w = text.split(',')
            size = int(h.strip()), int(w.strip())
            ok = size[0] >= 1 and size[1] >= 1
        elif text.strip():
            size = int(text.strip())
            ok = size >= 1
        else:
            size, ok = None, True
    except ValueError:
        ok = False
    if not ok:
        raise SystemExit("--out_size must be 'H,W', one positive integer (the shorter side) or empty (got {!r})".format(text))
    return size


def members_to_process(x_namelist, y_folder, out_folder):
    """-> [(image member, mask member, sample name)] in archive order (convert_isic.py:36-46)"""
    import os
    out = []
    for x_path in x_namelist:
        stem, ext = os.path.splitext(x_path)
        if ext.lower() == '.jpg' and not stem.lower().endswith('_superpixels'):
            x_name = os.path.splitext(os.path.split(x_path)[1])[0]
            out.append((x_path, '{}/{}_segmentation.png'.format(y_folder, x_name), '{}/{}'.format(out_folder, x_name)))
    return out


def target_size(h, w, out_size):
    """the size a (h, w) sample is resized to: None keeps it, (H, W) is fixed, an integer is the shorter side"""
    if out_size is None:
        return h, w
    if isinstance(out_size, tuple):
        return out_size
    s = float(out_size) / float(min(h, w))
    return int(round(h * s)), int(round(w * s))


def plan_chunks(sizes, chunk_bytes):
    """sizes [(H, W)] -> [(first, last)] runs of consecutive samples whose decoded pixels (4 bytes each: image and mask) fit
    chunk_bytes; a run holds at least one sample. Sizes may differ inside a run."""
    chunks, first = [], 0
    while first < len(sizes):
        last, used = first, 0
        while last < len(sizes) and (last == first or used + sizes[last][0] * sizes[last][1] * 4 <= int(chunk_bytes)):
            used += sizes[last][0] * sizes[last][1] * 4
            last += 1
        chunks.append((first, last))
        first = last
    return chunks


def same_size_runs(sizes):
    """[(H, W)] -> [(first, last)] maximal runs of consecutive equal sizes"""
    runs, first = [], 0
    for i in range(1, len(sizes) + 1):
        if i == len(sizes) or sizes[i] != sizes[first]:
            runs.append((first, i))
            first = i
    return runs


def check_request(out_size, items, x_sizes, y_sizes):
    """The refusals that need the archives' headers only -> None, or raises SystemExit"""
    for (x_name, y_name, _), xs, ys in zip(items, x_sizes, y_sizes):
        if xs != ys:
            raise SystemExit('{} is {}x{} but its mask {} is {}x{}'.format(x_name, xs[0], xs[1], y_name, ys[0], ys[1]))
        ho, wo = target_size(xs[0], xs[1], out_size)
        if ho > xs[0] or wo > xs[1] or ho < 1 or wo < 1:
            raise SystemExit('{} is {}x{}: --out_size asks for {}x{}, larger than the source along an axis (the area filter only '
                             'shrinks)'.format(x_name, xs[0], xs[1], ho, wo))


def mean_std_from_sums(sum_p, sum_p2, n_pixels):
    """Python integers [3], [3] and the pixel count -> float64 (rgb_mean, rgb_std) of p / 255 (convert_isic.py:67-73)"""
    import numpy as np
    mean = np.array([s / (255.0 * n_pixels) for s in sum_p], dtype=np.float64)
    mean_sq = np.array([s / (255.0 * 255.0 * n_pixels) for s in sum_p2], dtype=np.float64)
    return mean, np.sqrt(mean_sq - mean * mean)


def convert_archives(isic_zips_dir, out_size='248,248', chunk_bytes=DEFAULT_CHUNK_BYTES):
    """The whole conversion -> dict(n_samples, out_path, rgb_mean, rgb_std, seconds=dict(decode, device, encode_write)). Raises
    SystemExit with the reason for everything it refuses; the refusals come before the GPU is touched."""
    import io
    import os
    import pickle
    import time
    import zipfile
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    from PIL import Image

    from . import settings
    from .datapipe import isic2017_dataset, seg_data
    from .resident_pool import decode_threads

    out_size = parse_out_size(out_size) if (out_size is None or isinstance(out_size, str)) else out_size
    try:
        out_path = isic2017_dataset._get_isic2017_path(exists=False)
    except settings.DataPathError as e:
        raise SystemExit('{} -- `isic2017=<path of the .zip to write>` is where the converted archive goes.'.format(e))
    for x_zip_name, y_zip_name, _, _ in ARCHIVES:
        for name in (x_zip_name, y_zip_name):
            if not os.path.isfile(os.path.join(isic_zips_dir, name)):
                raise SystemExit('{} does not exist'.format(os.path.join(isic_zips_dir, name)))
    # the archives are read as a ZIP data source reads its own: one ZipFile each for all the threads, raw bytes under a lock
    items, zips = [], []
    for x_zip_name, y_zip_name, y_folder, split in ARCHIVES:
        x_zip = seg_data.ZipDataSource(os.path.join(isic_zips_dir, x_zip_name))
        y_zip = seg_data.ZipDataSource(os.path.join(isic_zips_dir, y_zip_name))
        found = members_to_process(x_zip.zip_file.namelist(), y_folder, split)
        if not found:
            raise SystemExit('{} holds no .jpg members'.format(os.path.join(isic_zips_dir, x_zip_name)))
        y_members = set(y_zip.zip_file.namelist())
        for x_name, y_name, _ in found:
            if y_name not in y_members:
                raise SystemExit('{} has no mask: {} is not in {}'.format(x_name, y_name, os.path.join(isic_zips_dir, y_zip_name)))
        items += found
        zips += [(x_zip, y_zip)] * len(found)
    n_train = sum(1 for it in items if it[2].startswith('train/'))

    with ThreadPoolExecutor(max_workers=decode_threads()) as ex:
        x_sizes = list(ex.map(lambda k: zips[k][0].member_size(items[k][0]), range(len(items))))
        y_sizes = list(ex.map(lambda k: zips[k][1].member_size(items[k][1]), range(len(items))))
        check_request(out_size, items, x_sizes, y_sizes)

        # nothing above has touched the GPU
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise SystemExit('convert_isic needs a GPU: the resize runs on the device only')
        device = torch.device('cuda', torch.cuda.current_device())

        out_dir = os.path.dirname(out_path)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        print('Writing data to {}'.format(out_path))
        seconds = dict(decode=0.0, device=0.0, encode_write=0.0)
        sum_p, sum_p2, n_pixels = [0, 0, 0], [0, 0, 0], 0
        with zipfile.ZipFile(out_path, 'w') as out_zip:
            for first, last in plan_chunks(x_sizes, chunk_bytes):
                k = last - first
                # one pinned staging pair per run of equally sized samples: the decoders write into it, and it goes over in one copy
                # (pinning is part of the price of the transfer: its time is booked under `device`)
                t_pin = time.time()
                runs = same_size_runs(x_sizes[first:last])
                stage_x, stage_y, slot = [], [], {}
                for r, (r0, r1) in enumerate(runs):
                    h, w = x_sizes[first + r0]
                    stage_x.append(torch.empty((r1 - r0, h, w, 3), dtype=torch.uint8, pin_memory=True))
                    stage_y.append(torch.empty((r1 - r0, h, w), dtype=torch.uint8, pin_memory=True))
                    slot.update({i: (r, i - r0) for i in range(r0, r1)})
                views_x, views_y = [t.numpy() for t in stage_x], [t.numpy() for t in stage_y]

                def decode(i):
                    (x_name, y_name, _), (x_zip, y_zip), (h, w) = items[first + i], zips[first + i], x_sizes[first + i]
                    x = np.asarray(x_zip.get_pil_image(x_name))
                    y = np.asarray(y_zip.get_pil_image(y_name))
                    if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
                        raise ValueError('{}: a 3-channel 8-bit image is expected, it decodes to {} {}'.format(x_name, x.dtype, x.shape))
                    if y.dtype != np.uint8 or y.ndim != 2:
                        raise ValueError('{}: a 2-D 8-bit mask is expected, it decodes to {} {}'.format(y_name, y.dtype, y.shape))
                    if x.shape != (h, w, 3) or y.shape != (h, w):
                        raise ValueError('{}: decodes to {} / {}, its header says {}x{}'.format(x_name, x.shape, y.shape, h, w))
                    r, j = slot[i]
                    views_x[r][j], views_y[r][j] = x, y

                t0 = time.time()
                list(ex.map(decode, range(k)))
                t1 = time.time()
                x_small, y_small = [None] * k, [None] * k
                for r, (r0, r1) in enumerate(runs):
                    h, w = x_sizes[first + r0]
                    ho, wo = target_size(h, w, out_size)
                    xs, ys = stage_x[r].to(device), stage_y[r].to(device)
                    xr, yr = ops.resize_area_u8(xs, ho, wo), ops.resize_area_u8(ys, ho, wo)
                    stats = ops.sum_sumsq_u8(xr).cpu().tolist()
                    xr, yr = xr.cpu().numpy(), yr.cpu().numpy()
                    for i in range(r0, r1):
                        x_small[i], y_small[i] = xr[i - r0], yr[i - r0]
                        if first + i < n_train:                                # the training samples come first
                            for ch in range(3):
                                sum_p[ch] += int(stats[i - r0][ch])
                                sum_p2[ch] += int(stats[i - r0][3 + ch])
                            n_pixels += ho * wo
                    del xs, ys
                del stage_x, stage_y, views_x, views_y
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
                seconds['device'] += (t2 - t1) + (t0 - t_pin)
                seconds['encode_write'] += t3 - t2
            rgb_mean, rgb_std = mean_std_from_sums(sum_p, sum_p2, n_pixels)
            out_zip.writestr('rgb_mean_std.pkl', pickle.dumps(dict(rgb_mean=rgb_mean, rgb_std=rgb_std)))
    print('{} samples ({} training), out_size {}: decode {:.1f}s, device {:.1f}s, encode and write {:.1f}s'.format(
        len(items), n_train, out_size, seconds['decode'], seconds['device'], seconds['encode_write']))
    return dict(n_samples=len(items), out_path=out_path, rgb_mean=rgb_mean, rgb_std=rgb_std, seconds=seconds)


@click.command(help='ISIC 2017 archive for the trainers from the four official downloads in ISIC_ZIPS_DIR; the area resize and the '
                    'image statistics run on the device. The resize is an exact integer area filter, not cv2.INTER_AREA: see the '
                    'module docstring.')
@click.argument('isic_zips_dir', type=click.Path(readable=True))
@click.option('--out_size', type=str, default='248,248')
def convert_isic(isic_zips_dir, out_size):
    convert_archives(isic_zips_dir, out_size)


if __name__ == '__main__':
    convert_isic()
