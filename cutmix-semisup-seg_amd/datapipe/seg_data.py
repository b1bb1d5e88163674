"""
The parts of the reference's datapipe/seg_data.py the device-side data path needs: the `DataSource` base (prediction files,
default statistics), `ZipDataSource` (samples that are members of one ZIP archive, read from many threads), the endless sampler
and -- in place of `DataLoader` + `SegCollate` -- the index streams and the canvas geometry of variable-sized evaluation batches.

Index streams. The reference samples with `RepeatSampler(SubsetRandomSampler(ndx))` through a `DataLoader`
(train_seg_semisup_mask_mt.py:203-212, 251-253): an endless chain of `torch.randperm` permutations drawn from torch's GLOBAL
generator, cut into consecutive batches that run across permutation boundaries; a loader's iterator draws one int64 (its base
seed) from the same generator when it is created (`iter(loader)`), before any permutation. `IndexStream` is exactly that with
`torch.utils.data.SubsetRandomSampler` itself and no loader, worker process or sample: it yields lists of indices. Streams
that share a `RepeatSampler` (the two unsupervised loaders) iterate it independently, as the loaders do.
"""
import itertools
import math
import os

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Sampler


class DataSource(object):
    """What the trainer asks of any data source beyond its index arrays (seg_data.py:112-124)."""

    def save_prediction_by_index(self, out_dir, pred_y_arr, sample_index):
        """<out_dir>/<sample name>.png, a 32-bit integer image (PIL mode 'I') of the predicted class map, as the reference
        writes it"""
        path = os.path.join(out_dir, self.sample_names[sample_index] + '.png')
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.asarray(pred_y_arr, dtype=np.uint32)).save(path)

    def get_mean_std(self):
        """ImageNet channel statistics, the default of every source"""
        return np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


_PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def labels_from_pil(img, name):
    """A decoded label image -> uint8 (H, W), the values it stores. 8-bit greyscale / palette PNGs and 16- / 32-bit integer ones
    both occur (the reference's Cityscapes converter saved a uint32 array); a value that does not fit a byte is refused, naming
    the member."""
    if img.mode not in ('L', 'P', 'I', 'I;16', 'I;16B', 'I;16L'):
        raise ValueError('{}: a greyscale, palette or integer label map is expected, got mode {}'.format(name, img.mode))
    arr = np.asarray(img)
    if arr.dtype != np.uint8:
        if arr.size and (int(arr.max()) > 255 or int(arr.min()) < 0):
            raise ValueError('{}: label values {}..{} do not fit a byte (0..255 is what the label pipeline carries)'.format(
                name, int(arr.min()), int(arr.max())))
        arr = arr.astype(np.uint8)
    return np.ascontiguousarray(arr)


def png_size(head):
    """(H, W) from the first 24 bytes of a PNG file, or None when they are not a PNG header"""
    import struct
    if len(head) >= 24 and head[:8] == _PNG_SIGNATURE and head[12:16] == b'IHDR':
        w, h = struct.unpack('>II', head[16:24])
        return int(h), int(w)
    return None


class ZipDataSource(DataSource):
    """A data source whose samples are members of one ZIP archive (seg_data.py:156-173): the base of the CamVid, Cityscapes and
    ISIC 2017 sources. A subclass fills `x_names` / `y_names` (member names, one per sample) and may override `map_labels`.

    The pool decodes on up to 16 threads at once. One `ZipFile` serves them all: the raw bytes of a member are read under a
    lock, and the decoding -- where the time goes, and where PIL lets go of the interpreter lock -- runs outside it."""

    def __init__(self, zip_path):
        import threading
        import zipfile
        self.zip_path = zip_path
        self.zip_file = zipfile.ZipFile(zip_path, 'r')
        self._zip_lock = threading.Lock()

    def __len__(self):
        return len(self.x_names)

    def _read_file_from_zip_as_bytes(self, name, n_bytes=-1):
        """the first `n_bytes` of a member (all of it with -1)"""
        with self._zip_lock:
            with self.zip_file.open(name) as f:
                return f.read(n_bytes)

    def get_pil_image(self, name):
        import io
        img = Image.open(io.BytesIO(self._read_file_from_zip_as_bytes(name)))
        img.load()
        return img

    def get_image_size(self, sample_i):
        return self.member_size(self.x_names[sample_i])

    def member_size(self, name):
        """-> (H, W) of an image member from its PNG header (the first 24 bytes): nothing is decoded"""
        size = png_size(self._read_file_from_zip_as_bytes(name, 24))
        if size is None:                                        # not a PNG: let PIL find the size in the whole member
            import io
            with Image.open(io.BytesIO(self._read_file_from_zip_as_bytes(name))) as img:
                size = int(img.size[1]), int(img.size[0])
        return size

    def get_image_arr(self, sample_i):
        """-> uint8 (H, W, 3) RGB"""
        img = self.get_pil_image(self.x_names[sample_i])
        return np.ascontiguousarray(np.asarray(img.convert('RGB'), dtype=np.uint8))

    def get_raw_labels_arr(self, sample_i):
        """-> uint8 (H, W): the values stored in the label member (labels_from_pil)"""
        name = self.y_names[sample_i]
        return labels_from_pil(self.get_pil_image(name), name)

    def map_labels(self, y):
        """stored values -> class indices (255 = void); the identity here"""
        return y

    def get_labels_arr(self, sample_i):
        """-> uint8 (H, W) class indices, 255 = void"""
        return np.ascontiguousarray(self.map_labels(self.get_raw_labels_arr(sample_i)), dtype=np.uint8)


def hold_out_split(train_ndx, val_ndx, n_val, val_rng, trainval_perm):
    """The hold-out rule the Cityscapes and ISIC 2017 sources share (cityscapes_dataset.py:90-108): `trainval_perm` re-orders the
    training list; with n_val > 0 the validation list becomes the TEST set and the last n_val of the training list -- in that order,
    or else in one drawn from val_rng -- the validation set. -> (train_ndx, val_ndx, test_ndx or None)"""
    if trainval_perm is not None:
        if len(trainval_perm) != len(train_ndx):
            raise ValueError('trainval_perm has {} entries, the training list {}'.format(len(trainval_perm), len(train_ndx)))
        train_ndx = train_ndx[np.asarray(trainval_perm)]
    elif n_val > 0:
        train_ndx = train_ndx[val_rng.permutation(len(train_ndx))]
    if n_val > 0:
        return train_ndx[:-n_val], train_ndx[-n_val:], val_ndx
    return train_ndx, val_ndx, None


class RepeatSampler(Sampler):
    """Iterates `sampler` again and again -- `repeats` times, or for ever with -1 -- as ONE sequence: every pass calls the
    sampler's own `__iter__` (a fresh torch.randperm for SubsetRandomSampler) when the previous pass runs out (seg_data.py:
    281-308)."""

    def __init__(self, sampler, repeats=-1):
        if repeats != -1 and repeats < 1:
            raise ValueError('repeats: a positive count, or -1 for an endless stream')
        self.sampler, self.repeats = sampler, repeats

    def __iter__(self):
        passes = itertools.repeat(self.sampler) if self.repeats == -1 else itertools.repeat(self.sampler, self.repeats)
        return itertools.chain.from_iterable(passes)

    def __len__(self):
        return 2 ** 62 if self.repeats == -1 else len(self.sampler) * self.repeats


class _IndexStreamIter(object):
    def __init__(self, sampler, batch_size):
        self._it = iter(sampler)
        self._batch_size = batch_size
        # what DataLoader's iterator draws from the global generator at its creation (its base seed for workers)
        torch.empty((), dtype=torch.int64).random_()

    def __iter__(self):
        return self

    def __next__(self):
        batch = [int(i) for i in itertools.islice(self._it, self._batch_size)]
        if not batch:
            raise StopIteration
        return batch


class IndexStream(object):
    """`DataLoader(index_dataset, batch_size, sampler=sampler)` reduced to its indices: `iter(stream)` yields consecutive
    lists of `batch_size` indices of `sampler` (the last one of a finite sampler may be shorter, as with drop_last=False)."""

    def __init__(self, sampler, batch_size):
        self.sampler = sampler
        self.batch_size = int(batch_size)

    def __iter__(self):
        return _IndexStreamIter(self.sampler, self.batch_size)


def repeat_stream(ndx, batch_size):
    """-> (IndexStream, its RepeatSampler) over an endless shuffle of `ndx`"""
    sampler = RepeatSampler(torch.utils.data.SubsetRandomSampler([int(i) for i in ndx]))
    return IndexStream(sampler, batch_size), sampler


def eval_batches(ndx, batch_size):
    """`DataLoader(Subset(ds, ndx), batch_size)` of the evaluation pipeline (datapipe/datasets.py:103-113): index order, last
    batch short"""
    ndx = [int(i) for i in ndx]
    return [ndx[i:i + batch_size] for i in range(0, len(ndx), batch_size)]


def collate_geometry(sizes, block_size):
    """SegCollate for whole images of `sizes` [(H, W), ...] (seg_data.py:181-216, 246-273): the canvas is the batch maximum
    rounded up to `block_size`, every image is centred with dh // 2 rows above and dw // 2 columns to the left.
    -> (canvas (Hc, Wc), offsets [(top, left), ...])"""
    size = (0, 0)
    for h, w in sizes:
        size = max(size[0], int(h)), max(size[1], int(w))
    canvas = (round(math.ceil(size[0] / block_size[0]) * block_size[0]),
              round(math.ceil(size[1] / block_size[1]) * block_size[1]))
    offsets = [((canvas[0] - int(h)) // 2, (canvas[1] - int(w)) // 2) for h, w in sizes]
    return canvas, offsets
