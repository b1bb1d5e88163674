"""
Mirror of the reference's patch_dist.py on the device: the sliding-window distance of query patches to every patch of an image,
and the nearest same-class / other-class pixels that intra_inter_class_patch_dist.py takes from those maps.

The images are uint8 and the reference's `img_as_float` only divides by 255, so everything here is computed on integer grey levels
and is EXACT: for an anchor patch Q[n] (p_h x p_w x 3) and an image symmetric-padded by (p - 1) // 2 per axis,

    D2[n,i,j] = sum (Ipad[i+u, j+v, c] - Q[n,u,v,c])^2 = P2[i,j] + Q2[n] - 2 PQ[n,i,j]

with PQ a `valid` cross-correlation from an fp64 FFT (csrc/fft.hip), a few 1e-6 from an integer and rounded back to it
(csrc/patchdist.hip). The reference's distance is sqrt(D2) / 255. Every call reports the largest distance from an integer it saw
(`last_rounding_residual()`) and raises when that exceeds 0.25: exactness would no longer be certain.

The distance of a patch to the patches centred on its four neighbours (neighbouring_patch_distance_maps, the input-distribution
figure) needs no FFT: shifting a patch by one pixel makes D2 a p_h x p_w box sum of squared neighbour differences of the image
padded by (p - 1) // 2 + 1, which two running-sum passes in int64 give exactly (neighbour_sqr_distance_maps, csrc/patchdist.hip).

Deviations from the reference, all deliberate:
  * patch sizes are odd on both axes (ValueError otherwise): the reference's even-size geometry is off by one and nothing uses it
  * the FFT size per axis is the smallest power of two >= max(8, H + p - 1), at most 4096 (ValueError beyond)
  * ties: the reference's np.argsort is unstable, so its order among equal distances is arbitrary; here equal distances are ordered
    by ascending flat pixel index i * W + j (the selection key is D2 << 24 | flat index, hence H * W <= 2^24 and
    3 * 255^2 * p_h * p_w < 2^39)
  * sliding_window_distance_to_patch[es_generator] take uint8 arrays; a float image is a TypeError
  * neighbouring_patch_distance_maps and patch_average_distance_map take a uint8 image (a float image is a TypeError) and odd
    patch sizes, as above
  * a neighbouring-patch distance that is exactly 0 is returned as 0.0: the reference's float64 summed-area table of img_as_float
    values cancels to about +-1e-13 there, which its square root turns into noise of about 1e-6 or into NaN

Host functions (numpy) keep the reference's names and conventions: neighbouring_pixels_class_change, boundary_pixels, box_sum,
extract_patch, and choose_anchors_and_negatives, which is the closure of intra_inter_class_patch_dist.py:46-104 made a function.
"""
import numpy as np

NEIGHBOUR_OFFSETS = np.array([[0, -1], [0, 1], [-1, 0], [1, 0]])        # dir: 0 = left, 1 = right, 2 = above, 3 = below
PATCH_DTYPE = np.dtype([('img_off', '<i8'), ('hs', '<i4'), ('ws', '<i4'), ('cy', '<i4'), ('cx', '<i4')])    # == cms_pd_patch
KEY_INDEX_BITS = 24
KEY_SENTINEL = np.iinfo(np.int64).max
DEFAULT_CHUNK = 32
RESIDUAL_LIMIT = 0.25

_last_residual = 0.0


# ------------------------------------------------------------------------------------------------------------------ host
def neighbouring_pixels_class_change(y):
    """(left, right, up, down): four (H, W) bool maps; a pixel is set where it is not void (255) and its neighbour in that
    direction has another class that is not void either. The outermost ring is never set (patch_dist.py:5-24)."""
    y = np.asarray(y)
    h, w = y.shape
    centre = y[1:-1, 1:-1]
    maps = []
    for dy, dx in NEIGHBOUR_OFFSETS:
        neighbour = y[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
        change = np.zeros((h, w), dtype=bool)
        change[1:-1, 1:-1] = (centre != 255) & (neighbour != centre) & (neighbour != 255)
        maps.append(change)
    return tuple(maps)


def boundary_pixels(y):
    """(H, W) bool: the pixel has a neighbour of another class in at least one direction (patch_dist.py:27-36)"""
    left, right, up, down = neighbouring_pixels_class_change(y)
    return left | right | up | down


def box_sum(x, box_size):
    """(H, W) -> (H + 1 - b_h, W + 1 - b_w): the sum of every b_h x b_w window, from a summed-area table (patch_dist.py:39-54).
    Integer and bool input is summed in int64 or uint64, where the table is exact; float input in its own type, as the reference
    does."""
    x = np.asarray(x)
    bh, bw = int(box_size[0]), int(box_size[1])
    if x.ndim != 2 or bh < 1 or bw < 1 or bh > x.shape[0] or bw > x.shape[1]:
        raise ValueError('box_sum: a box of {} x {} does not fit an array of shape {}'.format(bh, bw, x.shape))
    if x.dtype.kind in 'bi':
        x = x.astype(np.int64)
    elif x.dtype.kind == 'u':
        x = x.astype(np.uint64)
    s = np.pad(np.cumsum(np.cumsum(x, axis=1), axis=0), [[1, 0], [1, 0]], mode='constant')
    return s[bh:, bw:] - s[:-bh, bw:] - s[bh:, :-bw] + s[:-bh, :-bw]


def extract_patch(image, patch_shape, yx):
    """the (p_h, p_w, ...) patch of `image` centred on yx = (row, col) (patch_dist.py:157-168); no padding: stay inside"""
    pad_h, pad_w = ((int(s) - 1) // 2 for s in patch_shape)
    row, col = int(yx[0]), int(yx[1])
    return image[row - pad_h:row + pad_h + 1, col - pad_w:col + pad_w + 1, ...]


def symmetric_index(i, n):
    """source index of position i of an axis of length n under numpy's `symmetric` padding (the edge pixel repeats), for any i,
    however many reflections away"""
    m = np.mod(np.asarray(i), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def check_patch_shape(patch_shape):
    ph, pw = int(patch_shape[0]), int(patch_shape[1])
    if ph < 1 or pw < 1 or ph % 2 == 0 or pw % 2 == 0:
        raise ValueError('patch sizes must be odd on both axes (got {} x {}): the even-size geometry of the reference is off by one '
                         'and is not built'.format(ph, pw))
    if 3 * 255 * 255 * ph * pw >= 1 << 39:
        raise ValueError('patch {} x {} is too large: 3 * 255^2 * p_h * p_w must stay below 2^39 for the selection key'.format(ph, pw))
    return ph, pw


def choose_anchors_and_negatives(labels_of, sample_indices, n_patches, patch_shape, rng):
    """
    Anchor pixels next to a class boundary, the negative being the neighbour across it (intra_inter_class_patch_dist.py:46-104).
    labels_of(img_i) -> (H, W) label map. Returns int rows [img_i, dir, y, x, cls]: per image and direction the boundary pixels in
    row-major order, kept where `pad + 1 < i < H - (pad + 1)` on both axes, then ONE rng.permutation(len)[:n_patches] draw.
    """
    pad_h, pad_w = ((int(s) - 1) // 2 for s in patch_shape)
    border_h, border_w = pad_h + 1, pad_w + 1
    rows = []
    for img_i in sample_indices:
        y = np.array(labels_of(int(img_i)))
        for dir_i, change in enumerate(neighbouring_pixels_class_change(y)):
            i, j = np.where(change)
            keep = (i > border_h) & (i < y.shape[0] - border_h) & (j > border_w) & (j < y.shape[1] - border_w)
            i, j = i[keep], j[keep]
            rows.append(np.stack([np.ones_like(i) * img_i, np.ones_like(i) * dir_i, i, j, y[i, j]], axis=1))
    rows = np.concatenate(rows, axis=0)
    return rows[rng.permutation(len(rows))[:n_patches]]


# ------------------------------------------------------------------------------------------------------------------ device
def last_rounding_residual():
    """the largest |PQ - rint(PQ)| of the last sqr_distance_maps / class_neighbours call (0.5 is where exactness breaks)"""
    return _last_residual


def fft2(x, inverse=False):
    """in-place 2-D FFT of a complex128 CUDA (B, FH, FW) tensor (ops.fft2)"""
    from . import ops
    return ops.fft2(x, inverse=inverse)


def select_k_smallest(keys, mask, k):
    """the k smallest keys of each row of int64 (N, M) `keys` among those `mask` (N, M) marks: (sorted (N, k) padded with
    KEY_SENTINEL, counts (N,)) -- ops.select_k_smallest"""
    from . import ops
    return ops.select_k_smallest(keys, k, mask=mask)


class PatchSet(object):
    """
    Anchor patches cut on the device from pool entries. rows: int (N, [img_i, dir, y, x, cls]) as choose_anchors_and_negatives
    returns them (img_i a sample index the pool holds). Patches are cut from the symmetric-padded entry, so any centre inside the
    image is valid. With `negatives` also the negative patch of each anchor (the neighbour across the boundary,
    NEIGHBOUR_OFFSETS[dir]) and its distance:
        q2              int64 CUDA (N,)   sum of squares of each anchor
        boundary_d2     int64 CUDA (N,)   squared anchor-negative distance in grey levels
        boundary_dists  float64 numpy     sqrt(boundary_d2) / 255, the reference's `boundary_dists`
    """

    def __init__(self, pool, rows, patch_shape, negatives=True):
        import torch
        from . import ops
        self.patch_shape = check_patch_shape(patch_shape)
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != 5 or len(rows) == 0:
            raise ValueError('PatchSet: rows must be a non-empty (N, [img_i, dir, y, x, cls]) array')
        self.rows = rows
        self.pool = pool
        entries = pool.entries_of(rows[:, 0])
        anchor = np.zeros(len(rows), dtype=PATCH_DTYPE)
        for f in ('img_off', 'hs', 'ws'):
            anchor[f] = pool.table[f][entries]
        negative = anchor.copy()
        anchor['cy'], anchor['cx'] = rows[:, 2], rows[:, 3]
        offsets = NEIGHBOUR_OFFSETS[rows[:, 1]]
        negative['cy'], negative['cx'] = rows[:, 2] + offsets[:, 0], rows[:, 3] + offsets[:, 1]
        for d in (anchor, negative) if negatives else (anchor,):
            if ((d['cy'] < 0) | (d['cy'] >= d['hs']) | (d['cx'] < 0) | (d['cx'] >= d['ws'])).any():
                raise ValueError('PatchSet: a patch centre (or its neighbour across the boundary) lies outside its image')
        dev = pool.device
        self.n = len(rows)
        self.desc = torch.from_numpy(anchor.view(np.uint8).reshape(self.n, PATCH_DTYPE.itemsize).copy()).to(dev)
        self.desc_negative = torch.from_numpy(negative.view(np.uint8).reshape(self.n, PATCH_DTYPE.itemsize).copy()).to(dev)
        self.cls = torch.from_numpy(np.ascontiguousarray(rows[:, 4], dtype=np.int32)).to(dev)
        self.q2 = ops.pd_patch_sqdiff(pool.image_buffer, self.desc, None, self.n, self.patch_shape)
        self.boundary_d2 = self.boundary_dists = None
        if negatives:
            self.boundary_d2 = ops.pd_patch_sqdiff(pool.image_buffer, self.desc, self.desc_negative, self.n, self.patch_shape)
            self.boundary_dists = np.sqrt(self.boundary_d2.cpu().numpy().astype(np.float64)) / 255.0

    def __len__(self):
        return self.n

    @classmethod
    def from_arrays(cls, patches, device):
        """patches given as a uint8 (N, p_h, p_w, 3) array: each becomes a pool entry of its own, cut whole about its centre"""
        from .resident_pool import ResidentPool, ArraySource
        patches = np.asarray(patches)
        if patches.dtype != np.uint8 or patches.ndim != 4 or patches.shape[3] != 3:
            raise TypeError('patches must be a uint8 (N, p_h, p_w, 3) array')
        ph, pw = check_patch_shape(patches.shape[1:3])
        pool = ResidentPool(ArraySource(list(patches)), range(len(patches)), device, with_labels=False)
        rows = np.array([[i, 0, (ph - 1) // 2, (pw - 1) // 2, 0] for i in range(len(patches))])
        return cls(pool, rows, (ph, pw), negatives=False)


class _ImageSide(object):
    """what a distance map needs of the image alone: its spectrum (3, FH, FW), the box sums P2 (H, W), its label map"""

    def __init__(self, pool, sample_i, patch_shape):
        import torch
        from . import ops, _lib
        ph, pw = patch_shape
        e = int(pool.entries_of([sample_i])[0])
        t = pool.table[e]
        self.h, self.w = int(t['hs']), int(t['ws'])
        if self.h * self.w > 1 << KEY_INDEX_BITS:
            raise ValueError('image {} x {} has more than 2^24 pixels: the flat index does not fit the selection key'.format(
                self.h, self.w))
        hp, wp = self.h + ph - 1, self.w + pw - 1
        self.fft_shape = (ops.fft_size(hp), ops.fft_size(wp))
        dev = pool.device
        self.spectrum = torch.empty((3,) + self.fft_shape, dtype=torch.complex128, device=dev)
        sq = torch.empty((hp, wp), dtype=torch.int64, device=dev)
        entry = _lib.StageEntry(int(t['img_off']), int(t['lab_off']), self.h, self.w)
        ops.pd_load_image(pool.image_buffer, entry, patch_shape, self.fft_shape, self.spectrum, sq)
        ops.fft2(self.spectrum)
        # P2: the box sum of sum_c I^2 over p_h x p_w, once per image (plumbing: an int64 summed-area table)
        c = torch.nn.functional.pad(sq.cumsum(0).cumsum(1), (1, 0, 1, 0))
        self.p2 = (c[ph:, pw:] - c[:-ph, pw:] - c[ph:, :-pw] + c[:-ph, :-pw]).contiguous()
        assert tuple(self.p2.shape) == (self.h, self.w)
        self.labels = None
        if pool.label_buffer is not None:
            o = int(t['lab_off'])
            self.labels = pool.label_buffer[o:o + self.h * self.w]


class SpectrumCache(object):
    """the packed spectra of one chunk of patches, per FFT size: images of a data set share a handful of sizes, so a chunk's
    patches are transformed once per size, not once per image"""

    def __init__(self, patches, first, last):
        self.patches, self.first, self.last = patches, first, last
        self._by_shape = {}

    def get(self, fft_shape):
        import torch
        from . import ops
        if fft_shape not in self._by_shape:
            p, n = self.patches, self.last - self.first
            pairs = (n + 1) // 2
            spec = torch.empty((pairs, 3) + tuple(fft_shape), dtype=torch.complex128, device=p.pool.device)
            ops.pd_load_patches(p.pool.image_buffer, p.desc[self.first:self.last], n, p.patch_shape, fft_shape, spec)
            ops.fft2(spec.view((pairs * 3,) + tuple(fft_shape)))
            self._by_shape[fft_shape] = spec
        return self._by_shape[fft_shape]


def chunks_of(patches, chunk_size):
    chunk_size = int(chunk_size)
    if chunk_size < 1:
        raise ValueError('chunk_size must be positive')
    return [SpectrumCache(patches, i, min(i + chunk_size, len(patches))) for i in range(0, len(patches), chunk_size)]


def _finish_chunk(img, cache, residual_bits, d2=None, keys=None):
    """the correlation of one chunk with one image, finished into d2 and / or keys (views of the chunk's rows)"""
    import torch
    from . import ops
    spec = cache.get(img.fft_shape)
    corr = torch.empty((spec.shape[0],) + img.fft_shape, dtype=torch.complex128, device=spec.device)
    ops.pd_spectrum_product(img.spectrum, spec, corr)
    ops.fft2(corr, inverse=True)
    ops.pd_finish(corr, img.p2, cache.patches.q2[cache.first:cache.last], residual_bits, d2=d2, keys=keys)


def _read_residual(residual_bits):
    global _last_residual
    import torch
    _last_residual = float(residual_bits.view(torch.float64).item())
    if not _last_residual <= RESIDUAL_LIMIT:
        raise ArithmeticError('patch_dist: a cross-correlation came out {} away from an integer (limit {}): the squared distances '
                              'are no longer certain to be exact'.format(_last_residual, RESIDUAL_LIMIT))


def sqr_distance_maps(pool, sample_i, patches, chunk_size=DEFAULT_CHUNK):
    """int64 CUDA (N, H, W): the exact squared distance, in grey levels, of every patch of `patches` to the patch centred on every
    pixel of sample `sample_i` of `pool`. Patches go through in chunks of `chunk_size`, which bounds the workspace."""
    import torch
    img = _ImageSide(pool, sample_i, patches.patch_shape)
    d2 = torch.empty((len(patches), img.h, img.w), dtype=torch.int64, device=pool.device)
    residual_bits = torch.zeros((1,), dtype=torch.int64, device=pool.device)
    for cache in chunks_of(patches, chunk_size):
        _finish_chunk(img, cache, residual_bits, d2=d2[cache.first:cache.last])
    _read_residual(residual_bits)
    return d2


def neighbour_sqr_distance_maps(pool, sample_i, patch_shape):
    """int64 CUDA (4, H, W): the exact squared distance, in grey levels, between the patch centred on every pixel of sample
    `sample_i` of `pool` and the patches centred on its left, right, upper and lower neighbour (NEIGHBOUR_OFFSETS order), all cut
    from the sample symmetric-padded by (p - 1) // 2 + 1. Integer sums, no atomics: exact, and equal on every call."""
    from . import ops, _lib
    patch_shape = check_patch_shape(patch_shape)
    t = pool.table[int(pool.entries_of([sample_i])[0])]
    entry = _lib.StageEntry(int(t['img_off']), int(t['lab_off']), int(t['hs']), int(t['ws']))
    return ops.pd_neighbour_maps(pool.image_buffer, entry, patch_shape)


class Neighbours(object):
    """class_neighbours' result for N patches: sorted keys (N, k) int64 (D2 << 24 | y * W + x, KEY_SENTINEL past the count) and
    counts (N,), for the same-class (`intra`) and the other-class (`inter`) pixels of one image of width `width`"""

    def __init__(self, intra_keys, intra_count, inter_keys, inter_count, width):
        self.intra_keys, self.intra_count, self.inter_keys, self.inter_count = intra_keys, intra_count, inter_keys, inter_count
        self.width = width

    def lists(self):
        """per patch (intra, inter), each an int64 numpy (m, [D2, y, x]) in ascending order"""
        out = []
        sides = [(self.intra_keys.cpu().numpy(), self.intra_count.cpu().numpy()), (self.inter_keys.cpu().numpy(), self.inter_count.cpu().numpy())]
        for n in range(len(sides[0][0])):
            out.append(tuple(unpack_keys(keys[n, :int(count[n])], self.width) for keys, count in sides))
        return out


def unpack_keys(keys, width):
    keys = np.asarray(keys, dtype=np.int64)
    flat = keys & ((1 << KEY_INDEX_BITS) - 1)
    return np.stack([keys >> KEY_INDEX_BITS, flat // width, flat % width], axis=1)


def class_neighbours(pool, sample_i, patches, k, chunk_size=DEFAULT_CHUNK, chunks=None):
    """For each patch the k nearest pixels of sample `sample_i` whose label equals the patch's class (`intra`) and the k nearest
    whose label is another class and not 255 (`inter`): (D2, y, x) ascending, ties by flat pixel index; fewer than k candidates
    give fewer results. No sort of the map: a radix select over the masked keys (csrc/patchdist.hip). `chunks` (chunks_of) lets a
    caller that visits many images keep the patch spectra."""
    import torch
    from . import ops
    if pool.label_buffer is None:
        raise ValueError('class_neighbours: the pool holds no labels')
    img = _ImageSide(pool, sample_i, patches.patch_shape)
    residual_bits = torch.zeros((1,), dtype=torch.int64, device=pool.device)
    parts = []
    for cache in (chunks if chunks is not None else chunks_of(patches, chunk_size)):
        n = cache.last - cache.first
        keys = torch.empty((n, img.h * img.w), dtype=torch.int64, device=pool.device)
        _finish_chunk(img, cache, residual_bits, keys=keys)
        cls = patches.cls[cache.first:cache.last]
        parts.append(ops.select_k_smallest(keys, k, labels=img.labels, cls=cls) +
                     ops.select_k_smallest(keys, k, labels=img.labels, cls=cls, inter=True))
    _read_residual(residual_bits)
    return Neighbours(*[torch.cat([p[i] for p in parts]) for i in range(4)], width=img.w)


def merge_best(run_keys, run_img, new_keys, new_img_i, k):
    """The running best-k per patch across images, ordered by (D2, visit order, flat index): run_keys / run_img (N, <= k) hold what
    earlier images gave (sorted, KEY_SENTINEL where empty), new_keys (N, k) what this image gives. A stable sort by D2 alone keeps
    earlier images first among equal distances and, within this image, the ascending flat index. -> (keys, img) (N, k)"""
    import torch
    keys = torch.cat([run_keys, new_keys], dim=1)
    img = torch.cat([run_img, torch.full_like(new_keys, int(new_img_i))], dim=1)
    d2 = torch.where(keys == KEY_SENTINEL, keys, keys >> KEY_INDEX_BITS)
    order = torch.sort(d2, dim=1, stable=True).indices[:, :k]
    return torch.gather(keys, 1, order), torch.gather(img, 1, order)


# ------------------------------------------------------------------------------------------------------- reference drop-ins
def _need_uint8(what, a):
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError('{} must be uint8, got {}: the device path computes on integer grey levels, which is what makes it exact; '
                        'pass the stored image, not the output of img_as_float (the distances returned are already in its units)'
                        .format(what, a.dtype))
    return a


def sliding_window_distance_to_patches_generator(image, patches):
    """uint8 image (H, W, 3) and patches (N, p_h, p_w, 3) -> yields N float64 (H, W) maps: the Euclidean distance, in the units of
    img_as_float, of each patch to the patch centred on every pixel of the symmetric-padded image (patch_dist.py:130-154)"""
    import torch
    from .resident_pool import ResidentPool, ArraySource
    image, patches = _need_uint8('image', image), _need_uint8('patches', patches)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('image must be (H, W, 3)')
    dev = torch.device('cuda', torch.cuda.current_device())
    pool = ResidentPool(ArraySource([image]), [0], dev, with_labels=False)
    d2 = sqr_distance_maps(pool, 0, PatchSet.from_arrays(patches, dev))
    for n in range(d2.shape[0]):
        yield np.sqrt(d2[n].cpu().numpy().astype(np.float64)) / 255.0


def sliding_window_distance_to_patch(image, patch):
    """one patch (p_h, p_w, 3): the (H, W) map (patch_dist.py:107-127)"""
    patch = _need_uint8('patch', patch)
    return next(sliding_window_distance_to_patches_generator(image, patch[None]))


def neighbouring_patch_distance_maps(x, patch_size):
    """uint8 image (H, W, 3) -> (left, right, up, down): four float64 (H, W) maps, the Euclidean distance, in the units of
    img_as_float, between the patch centred on a pixel and the patch centred on its neighbour in that direction
    (patch_dist.py:57-87). Exactly sqrt(D2) / 255 of the integer D2, so 0.0 where the two patches are equal."""
    import torch
    from .resident_pool import ResidentPool, ArraySource
    x = _need_uint8('image', x)
    patch_size = check_patch_shape(patch_size)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError('image must be (H, W, 3)')
    dev = torch.device('cuda', torch.cuda.current_device())
    pool = ResidentPool(ArraySource([x]), [0], dev, with_labels=False)
    d2 = neighbour_sqr_distance_maps(pool, 0, patch_size).cpu().numpy()
    return tuple(np.sqrt(d2[k].astype(np.float64)) / 255.0 for k in range(4))


def patch_average_distance_map(x, patch_size):
    """the mean of the four maps of neighbouring_patch_distance_maps, added in the reference's order (patch_dist.py:90-104)"""
    left_d, right_d, up_d, down_d = neighbouring_patch_distance_maps(x, patch_size)
    return (left_d + right_d + up_d + down_d) * 0.25
