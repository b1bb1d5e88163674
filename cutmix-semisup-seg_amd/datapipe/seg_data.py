"""
The parts of the reference's datapipe/seg_data.py the device-side data path needs: the `DataSource` base (prediction files,
default statistics), the endless sampler and -- in place of `DataLoader` + `SegCollate` -- the index streams and the canvas
geometry of variable-sized evaluation batches.

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
