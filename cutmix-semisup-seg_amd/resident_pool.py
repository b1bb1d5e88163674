"""
A pool of VARIABLE-SIZED uint8 images (and label maps) resident in HBM: a data set is decoded once, at start-up, and every
training / evaluation batch is then gathered on the device by index (csrc/stage.hip through device_pipeline.DeviceAugmenter.stage
/ stage_eval) -- no per-iteration host image work, nothing but a parameter table and an index vector crosses PCIe.

Layout (what cms_stage_desc describes):
    image buffer   one uint8 tensor; entry e is [Hs][Ws][3] with dense rows (3 * Ws bytes) at byte offset img_off[e]
    label buffer   one uint8 tensor; entry e is [Hs][Ws] at byte offset lab_off[e]
    entry table    device array of cms_stage_entry {int64 img_off, int64 lab_off, int32 hs, int32 ws}
Every entry starts on a 16-byte boundary; offsets are 64-bit (Pascal VOC augmented: ~7 GB of pixels + 2.3 GB of labels). A
sample index that is asked for several times (the supervised subset is part of the unsupervised set) is stored once.

Decoding runs on a thread pool (PIL releases the GIL while it decodes) of at most min(16, CPUs this process may use) threads;
the upload goes chunk by chunk through one host staging buffer, so host memory holds a bounded part of the data set at a time.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ALIGN = 16
ENTRY_DTYPE = np.dtype([('img_off', '<i8'), ('lab_off', '<i8'), ('hs', '<i4'), ('ws', '<i4')])    # == cms_stage_entry
DEFAULT_CHUNK_BYTES = 256 << 20


def _align(v):
    return (int(v) + ALIGN - 1) // ALIGN * ALIGN


def plan_layout(sizes):
    """sizes [(Hs, Ws), ...] -> (entry table as a structured array, image buffer bytes, label buffer bytes)"""
    table = np.zeros(len(sizes), dtype=ENTRY_DTYPE)
    img_pos = lab_pos = 0
    for e, (hs, ws) in enumerate(sizes):
        hs, ws = int(hs), int(ws)
        if hs <= 0 or ws <= 0:
            raise ValueError('ResidentPool: entry {} has size {}x{}'.format(e, hs, ws))
        img_pos, lab_pos = _align(img_pos), _align(lab_pos)
        table[e] = (img_pos, lab_pos, hs, ws)
        img_pos += hs * ws * 3
        lab_pos += hs * ws
    return table, img_pos, lab_pos


def decode_threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


class ResidentPool(object):
    def __init__(self, ds, indices, device, with_labels=True, chunk_bytes=DEFAULT_CHUNK_BYTES):
        """ds: a data source with get_image_size(i) -> (H, W), get_image_arr(i) -> uint8 (H, W, 3), get_labels_arr(i) ->
        uint8 (H, W). indices: the sample indices to hold (any order, repeats stored once)."""
        self.device = torch.device(device)
        seen = {}
        for i in indices:
            seen.setdefault(int(i), len(seen))
        self.sample_indices = list(seen.keys())
        self._entry_of = seen
        self.with_labels = bool(with_labels)
        n = len(self.sample_indices)
        if n == 0:
            raise ValueError('ResidentPool: no samples')
        with ThreadPoolExecutor(max_workers=decode_threads()) as ex:
            sizes = list(ex.map(ds.get_image_size, self.sample_indices))
            self.table, img_bytes, lab_bytes = plan_layout(sizes)
            if not self.with_labels:
                self.table['lab_off'] = -1
            self.image_buffer = torch.zeros(img_bytes, dtype=torch.uint8, device=self.device)
            self.label_buffer = torch.zeros(lab_bytes, dtype=torch.uint8, device=self.device) if self.with_labels else None
            self._upload(ds, ex, int(chunk_bytes))
        self.table_dev = torch.from_numpy(self.table.view(np.uint8).copy()).to(self.device)

    # -- building
    def _upload(self, ds, ex, chunk_bytes):
        """Decode and upload runs of consecutive entries whose image bytes fit one staging buffer."""
        n = len(self.table)
        first = 0
        while first < n:
            last = first + 1
            base = int(self.table['img_off'][first])
            while last < n and int(self.table['img_off'][last]) + self._img_bytes(last) - base <= chunk_bytes:
                last += 1
            self._upload_run(ds, ex, first, last)
            first = last

    def _img_bytes(self, e):
        return int(self.table['hs'][e]) * int(self.table['ws'][e]) * 3

    def _upload_run(self, ds, ex, first, last):
        t = self.table
        ids = self.sample_indices[first:last]
        img_base = int(t['img_off'][first])
        img_end = int(t['img_off'][last - 1]) + self._img_bytes(last - 1)
        stage_img = np.zeros(img_end - img_base, dtype=np.uint8)
        stage_lab = None
        if self.with_labels:
            lab_base = int(t['lab_off'][first])
            lab_end = int(t['lab_off'][last - 1]) + self._img_bytes(last - 1) // 3
            stage_lab = np.zeros(lab_end - lab_base, dtype=np.uint8)

        def load(k):
            e = first + k
            hs, ws = int(t['hs'][e]), int(t['ws'][e])
            img = ds.get_image_arr(ids[k])
            if img.dtype != np.uint8 or img.shape != (hs, ws, 3):
                raise ValueError('ResidentPool: sample {} decodes to {} {}, its header says {}x{}'.format(
                    ids[k], img.dtype, img.shape, hs, ws))
            o = int(t['img_off'][e]) - img_base
            stage_img[o:o + hs * ws * 3] = img.reshape(-1)
            if stage_lab is not None:
                lab = ds.get_labels_arr(ids[k])
                if lab.dtype != np.uint8 or lab.shape != (hs, ws):
                    raise ValueError('ResidentPool: labels of sample {} are {} {}, the image is {}x{}'.format(
                        ids[k], lab.dtype, lab.shape, hs, ws))
                o = int(t['lab_off'][e]) - lab_base
                stage_lab[o:o + hs * ws] = lab.reshape(-1)
        list(ex.map(load, range(last - first)))
        self.image_buffer[img_base:img_end].copy_(torch.from_numpy(stage_img))
        if stage_lab is not None:
            self.label_buffer[lab_base:lab_end].copy_(torch.from_numpy(stage_lab))

    # -- lookups
    def __len__(self):
        return len(self.table)

    def entries_of(self, indices):
        """sample indices -> int32 pool entries (KeyError for a sample the pool does not hold)"""
        return np.array([self._entry_of[int(i)] for i in indices], dtype=np.int32)

    def sizes_of(self, indices):
        e = self.entries_of(indices)
        return [(int(self.table['hs'][k]), int(self.table['ws'][k])) for k in e]

    def image(self, sample_i):
        """the stored image of a sample, back on the host: uint8 (Hs, Ws, 3)"""
        e = self._entry_of[int(sample_i)]
        hs, ws, o = int(self.table['hs'][e]), int(self.table['ws'][e]), int(self.table['img_off'][e])
        return self.image_buffer[o:o + hs * ws * 3].cpu().numpy().reshape(hs, ws, 3)

    def labels(self, sample_i):
        if self.label_buffer is None:
            return None
        e = self._entry_of[int(sample_i)]
        hs, ws, o = int(self.table['hs'][e]), int(self.table['ws'][e]), int(self.table['lab_off'][e])
        return self.label_buffer[o:o + hs * ws].cpu().numpy().reshape(hs, ws)

    def nbytes(self):
        return int(self.image_buffer.numel()) + (int(self.label_buffer.numel()) if self.label_buffer is not None else 0)


class ArraySource(object):
    """A data source over arrays already in memory (tests, synthetic pools): images [uint8 (H, W, 3)], labels [uint8 (H, W)]"""

    def __init__(self, images, labels=None):
        self.images = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        self.labels_ = None if labels is None else [np.ascontiguousarray(a, dtype=np.uint8) for a in labels]

    def get_image_size(self, i):
        return self.images[i].shape[0], self.images[i].shape[1]

    def get_image_arr(self, i):
        return self.images[i]

    def get_labels_arr(self, i):
        return self.labels_[i]
