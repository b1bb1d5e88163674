"""
Geometry of an augmented PAIR of views (host, numpy only): the random draws of the reference's `transform_pair` methods, per
sample and in their order, and the matrices that go with them.

    transform choice     train_seg_semisup_aug_mt.py:129-144   Hung scale crop, else rotate / scale crop (when --aug_max_scale
                                                               != 1 or --aug_rot_mag != 0), else plain crop; then the flips
    plain crop           datapipe/seg_transforms_cv.py:135-166  pos0 = round(extra * U(0,1)^2); pos1 = clip(pos0 +
                                                               round(offset_range * U(-1,1)^2), 0, extra)
    Hung scale crop      :232-303   view 1 is cut at 1 / f_scale1 of the crop and resized: f_scale1 = 0.5 + randint(0, 11) / 10
    rotate / scale crop  :380-449   one (scale, angle) for both views, or one each with --aug_free_scale_rot
    flips                :498-538   binomial(1, 0.5, (2, 3)) & [hflip, vflip, hvflip]
    xf0_to_1             datapipe/seg_data.py:222-226   cv_to_torch(xf1_cv . xf0_cv^-1, crop): the theta of
                                                               F.affine_grid(align_corners=True) that warps view 0 into view 1

Matrices are `cv2.warpAffine`-style 2x3 float32 arrays composed in float32 with the conventions of datapipe/affine.py (x before
y, rotation [[c, s], [-s, c]]), as DeviceAugmenter.local_xf already does for a single view.

The views themselves are cut on the device by the staging kernel (csrc/stage.hip) that cuts single views: `pair_rows` turns one
drawn pair into two rows of its parameter table (include/cutmixseg.h, CMS_AUG_PARAMS), DeviceAugmenter.stage_pair adds the
colour draw of view 1 and launches it over both views of a batch.

    plain crop           two window rows: origin pos_v (relative to the unpadded source), size = crop
    Hung scale crop      view 0: window pos0 / crop; view 1: window pos1 / sc_size1, resized by the kernel, its validity mask
                         resized with INTER_NEAREST (:272; slot 23 = 1) where single views use INTER_LINEAR (:215)
    rotate / scale crop  two warp rows: the float64 inverse of the pre-flip xf_cv[v], always INTER_LINEAR (:426)
    flips                slots 4-6 of each row
"""
import numpy as np

F32 = np.float32
N_PARAMS = 24               # == CMS_AUG_PARAMS


def identity(n=1):
    m = np.zeros((n, 2, 3), dtype=F32)
    m[:, 0, 0] = m[:, 1, 1] = 1.0
    return m


def translation(xy):
    """(N,2) offsets (x, y) -> (N,2,3)"""
    xy = np.asarray(xy)
    m = identity(len(xy))
    m[:, :, 2] = xy
    return m


def scaling(xy):
    xy = np.asarray(xy)
    m = np.zeros((len(xy), 2, 3), dtype=F32)
    m[:, 0, 0] = xy[:, 0]
    m[:, 1, 1] = xy[:, 1]
    return m


def rotation(thetas):
    """counter-clockwise with +y pointing down: [[c, s], [-s, c]]"""
    thetas = np.asarray(thetas)
    m = np.zeros((len(thetas), 2, 3), dtype=F32)
    m[:, 0, 0] = m[:, 1, 1] = np.cos(thetas)
    m[:, 0, 1] = np.sin(thetas)
    m[:, 1, 0] = -np.sin(thetas)
    return m


def cat(*ms):
    """ms[0] . ms[1] . ... (the right-most acts first), N matrices at a time"""
    out = ms[0]
    for b in ms[1:]:
        lin = np.matmul(out[:, :, :2], b[:, :, :2])
        off = out[:, :, 2:3] + np.matmul(out[:, :, :2], b[:, :, 2:3])
        out = np.append(lin, off, axis=2)
    return out


def inverse(m):
    a = m[:, :, :2]
    rdet = 1.0 / (a[:, 0, 0] * a[:, 1, 1] - a[:, 1, 0] * a[:, 0, 1])
    inv = np.zeros_like(a)
    inv[:, 0, 0] = a[:, 1, 1] * rdet
    inv[:, 1, 1] = a[:, 0, 0] * rdet
    inv[:, 0, 1] = -a[:, 0, 1] * rdet
    inv[:, 1, 0] = -a[:, 1, 0] * rdet
    return np.append(inv, np.matmul(inv, -m[:, :, 2:3]), axis=2)


def flips(flags_xyd, size_hw):
    """(N,3) flags [x, y, transpose] for images of size (H, W) -> (N,2,3): transpose . T(size - 1 where flipped) . S(+-1)"""
    flags_xyd = np.asarray(flags_xyd, dtype=bool)
    sign = flags_xyd[:, :2] * -2 + 1
    shift = flags_xyd[:, :2] * (np.array(size_hw[::-1]).astype(float) - 1)
    swap = identity(len(flags_xyd))
    d = flags_xyd[:, 2]
    swap[d] = swap[d][:, ::-1, :]
    return cat(swap, translation(shift), scaling(sign))


def cv_to_torch(m, size_hw):
    """warpAffine matrices (they move the IMAGE) -> thetas of F.affine_grid / F.grid_sample with align_corners=True (they move
    the SAMPLING POINTS, in [-1, 1] coordinates): normalise . m^-1 . un-normalise, source and destination of `size_hw`"""
    sx, sy = float(size_hw[1] - 1) / 2.0, float(size_hw[0] - 1) / 2.0
    n = len(m)
    to_px = identity(n)
    to_px[:, 0, 0] = to_px[:, 0, 2] = sx
    to_px[:, 1, 1] = to_px[:, 1, 2] = sy
    to_unit = identity(n)
    to_unit[:, 0, 0] = 1.0 / sx
    to_unit[:, 1, 1] = 1.0 / sy
    to_unit[:, :, 2] = -1.0
    return cat(to_unit, inverse(m), to_px)


def xf0_to_1(xf0_cv, xf1_cv, size_hw):
    """(N,2,3) x2 -> the (N,2,3) float32 `xf0_to_1` of the reference's collate function"""
    return cv_to_torch(cat(xf1_cv, inverse(xf0_cv)), size_hw).astype(F32)


def inverse_slots(m):
    """A 2x3 warpAffine matrix -> slots 16..21 of a warp row, (a00 a01 a02 a10 a11 a12) of its inverse in float64 (cv2 inverts
    in double precision)"""
    m = np.asarray(m).astype(np.float64)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    inv2 = np.array([[m[1, 1], -m[0, 1]], [-m[1, 0], m[0, 0]]]) / det
    invt = -inv2 @ m[:, 2]
    return (inv2[0, 0], inv2[0, 1], invt[0], inv2[1, 0], inv2[1, 1], invt[1])


def pair_rows(info, crop_size):
    """One drawn pair (the parameter dict of PairGeometry.draw) -> float32 (2, N_PARAMS): the rows of the staging kernel's
    parameter table that cut view 0 and view 1. No colour change (slots 7-9 = 1, 11-13 = 0): DeviceAugmenter.stage_pair draws
    view 1's."""
    crop = (int(crop_size[0]), int(crop_size[1]))
    rows = np.zeros((2, N_PARAMS), dtype=F32)
    rows[:, 7:10] = 1.0
    if info['kind'] == 'warp':
        rows[:, 2:4] = crop
        rows[:, 15] = 1.0
        rows[:, 22] = 1.0                                  # an unlabelled pair is always INTER_LINEAR
        for v in range(2):
            rows[v, 16:22] = inverse_slots(info['xf_cv'][v])
    else:
        rows[0, 0:2], rows[1, 0:2] = info['pos0'], info['pos1']
        rows[:, 2:4] = crop
        if info['kind'] == 'hung':
            rows[1, 2:4] = info['sc_size1']
            rows[1, 23] = 1.0                              # view 1's mask is resized with INTER_NEAREST
    if 'flips' in info:
        rows[:, 4:7] = info['flips']
    return rows


class PairGeometry(object):
    """Draws the geometry of pairs of views cut from source images."""

    def __init__(self, crop_size, offset_range=16.0, scale_hung=False, max_scale=1.0, rot_mag=0.0, scale_non_uniform=False,
                 free_scale_rot=False, hflip=False, vflip=False, hvflip=False, rng=None):
        self.crop = np.array([int(crop_size[0]), int(crop_size[1])])
        self.offset = np.array([offset_range, offset_range])
        self.scale_hung, self.uniform_scale = bool(scale_hung), not scale_non_uniform
        self.rot_mag_rad = float(np.radians(rot_mag))
        self.log_max_scale = float(np.log(max_scale))
        self.warp = (not self.scale_hung) and (max_scale != 1.0 or rot_mag != 0.0)
        self.constrain = not free_scale_rot
        self.flip_flags = np.array([[hflip, vflip, hvflip]], dtype=bool)
        if hvflip and self.crop[0] != self.crop[1]:
            raise ValueError('aug_hvflip (transpose) needs a square crop')
        self._rng = rng

    @property
    def rng(self):
        if self._rng is None:
            self._rng = np.random.RandomState()
        return self._rng

    @staticmethod
    def _padding(img, need):
        """leading padding (y, x) of a source smaller than `need`, and the padded size"""
        pad = np.maximum(np.asarray(need) - img, 0)
        return pad // 2, img + pad

    def _crop_pair(self, img):
        lead, size = self._padding(img, self.crop)
        extra = size - self.crop
        pos0 = np.round(extra * self.rng.uniform(0.0, 1.0, size=(2,))).astype(int)
        pos1 = pos0 + np.round(self.offset * self.rng.uniform(-1.0, 1.0, size=(2,))).astype(int)
        pos1 = np.clip(pos1, np.array([0, 0]), extra)
        base = translation(np.array([lead[::-1], lead[::-1]])) if lead.any() else identity(2)
        xf = cat(translation(-np.stack([pos0[::-1], pos1[::-1]])), base)
        return xf, dict(kind='crop', pos0=pos0 - lead, pos1=pos1 - lead)

    def _hung_pair(self, img):
        f_scale1 = 0.5 + self.rng.randint(0, 11, size=(1 if self.uniform_scale else 2,)) / 10.0
        sc_size1 = np.round(self.crop / f_scale1).astype(int)
        biggest = np.maximum(self.crop, sc_size1)
        lead, size = self._padding(img, biggest)
        extra = size - biggest
        pos0 = np.round(extra * self.rng.uniform(0.0, 1.0, size=(2,))).astype(int)
        pos1 = pos0 + np.round(self.offset * self.rng.uniform(-1.0, 1.0, size=(2,))).astype(int)
        pos1 = np.clip(pos1, np.array([0, 0]), extra)
        pos0 = np.round(pos0 + biggest * 0.5 - self.crop * 0.5).astype(int)
        pos1 = np.round(pos1 + biggest * 0.5 - sc_size1 * 0.5).astype(int)
        # view 1 is resized sc_size1 -> crop: scale out / in and the half-pixel shift (scale - 1) / 2 of cv2.resize
        factors = np.append(np.array([[1, 1]]), self.crop[None, ::-1].astype(float) / sc_size1[None, ::-1], axis=0)
        base = translation(np.array([lead[::-1], lead[::-1]])) if lead.any() else identity(2)
        xf = cat(translation((factors - 1.0) * 0.5), scaling(factors), translation(-np.stack([pos0[::-1], pos1[::-1]])), base)
        return xf, dict(kind='hung', pos0=pos0 - lead, pos1=pos1 - lead, sc_size1=sc_size1)

    def _warp_pair(self, img):
        lo, hi = -self.log_max_scale, self.log_max_scale
        k = 1 if self.constrain else 2
        if self.uniform_scale:
            scales = np.repeat(np.exp(self.rng.uniform(lo, hi, size=(k, 1))), 2, axis=1)
        else:
            scales = np.exp(self.rng.uniform(lo, hi, size=(k, 2)))
        thetas = self.rng.uniform(-self.rot_mag_rad, self.rot_mag_rad, size=(k,))
        if self.constrain:
            scales, thetas = np.repeat(scales, 2, axis=0), np.repeat(thetas, 2, axis=0)
        sc_size = self.crop / scales.min(axis=0)
        centre0 = np.maximum(img - sc_size, 0.0) * self.rng.uniform(0.0, 1.0, size=(2,)) + np.minimum(sc_size, img) * 0.5
        offset1 = np.round(self.offset * self.rng.uniform(-1.0, 1.0, size=(2,)))
        xf = cat(translation(self.crop[None, ::-1] * 0.5), translation(np.stack([np.zeros((2,)), offset1])[:, ::-1]),
                 rotation(thetas), scaling(scales[:, ::-1]), translation(-np.stack([centre0, centre0])[:, ::-1]))
        return xf, dict(kind='warp', scales_yx=scales, thetas=thetas, centre0=centre0, offset1=offset1)

    def draw(self, src_hw):
        """One pair. -> (xf_cv (2,2,3) float32: source image -> view 0 / view 1, xf0_to_1 (2,3) float32, the drawn parameters;
        their 'xf_cv' is the pair of matrices BEFORE the flips, which is what cuts the views: the flips come after the cut)"""
        img = np.array([int(src_hw[0]), int(src_hw[1])])
        if self.scale_hung:
            xf, info = self._hung_pair(img)
        elif self.warp:
            xf, info = self._warp_pair(img)
        else:
            xf, info = self._crop_pair(img)
        info['xf_cv'] = xf
        if self.flip_flags.any():
            f = (self.rng.binomial(1, 0.5, size=(2, 3)) != 0) & self.flip_flags
            xf = cat(flips(f, tuple(self.crop)), xf)
            info['flips'] = f
        return xf, xf0_to_1(xf[0:1], xf[1:2], tuple(self.crop))[0], info

    def draw_batch(self, n, src_hw):
        """`src_hw`: one (Hs, Ws) for the whole batch, or a list of n of them (a ragged batch); the pairs are drawn one after the
        other from the one generator, as the loader workers of the reference transform sample after sample.
        -> (xf0_to_1 (n,2,3) float32, xf_cv (n,2,2,3) float32, list of parameter dicts)"""
        sizes = [src_hw] * n if np.ndim(src_hw) == 1 else list(src_hw)
        if len(sizes) != n:
            raise ValueError('draw_batch: {} sizes for {} pairs'.format(len(sizes), n))
        out = [self.draw(s) for s in sizes]
        return np.stack([o[1] for o in out]), np.stack([o[0] for o in out]), [o[2] for o in out]
