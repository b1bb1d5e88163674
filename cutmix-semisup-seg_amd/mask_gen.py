"""
Mirror of the reference's mask_gen.py (BoxMaskGenerator + AddMaskParamsToBatch), MI355X-first.

The reference draws box parameters with numpy on the CPU (mask_gen.py:70-108), rasterises full-resolution float64
masks there (:110-116), ships N*H*W fp32 to the GPU every iteration (train_seg_semisup_mask_mt.py:331) and declares
`torch_masks_from_params` the identity (:119-120).

Here the random draws stay on the host with the SAME numpy call sequence (so a seeded RandomState gives the same
boxes, bit for bit), but what travels to the device is the (N, n_boxes, 4) int32 table of half-open ranges
[y0, y1, x0, x1]; kernels rasterise it on the fly (csrc/boxmask.hip, csrc/losses.hip). `generate_params` still
returns the reference's float64 (N,1,H,W) array for drop-in use; `generate_ranges` + `torch_masks_from_params`
is the device path.

CowMaskGenerator is not in the reference, which only carries its scaffolding (the abstract `torch_masks_from_params`,
`gaussian_kernels`): host draws of (p, sigma) per sample, the masks themselves made on the device (csrc/cowmask.hip).

ClassMixGenerator is not in the reference either: host draws of one key per sample and class, the masks cut along the teacher's
predicted class regions on the device (csrc/classmix.hip).
"""
import numpy as np
import torch

from . import ops


class MaskGenerator(object):
    """Mask Generator (abstract; mask_gen.py:10-23)"""

    def generate_params(self, n_masks, mask_shape, rng=None):
        raise NotImplementedError('Abstract')

    def append_to_batch(self, *batch):
        x = batch[0]
        params = self.generate_params(len(x), x.shape[2:4])
        return batch + (params,)

    def torch_masks_from_params(self, t_params, mask_shape, torch_device):
        raise NotImplementedError('Abstract')


def gaussian_kernels(sigma, max_sigma=None, truncate=4.0):
    """Rows of normalised 1-D Gaussian kernels, one per entry of `sigma` ((N,) array), all of the width the LARGEST sigma asks
    for (radius = int(truncate * max_sigma + 0.5)) -- mask_gen.py:26-43 of the reference, a host-side helper that nothing there
    calls; here it is the tap table of CowMaskGenerator."""
    sigma = np.asarray(sigma, dtype=np.float64)
    if max_sigma is None:
        max_sigma = sigma.max()
    radius = int(truncate * max_sigma + 0.5)
    offsets = np.arange(-radius, radius + 1, dtype=np.float64)[None, :]
    weights = np.exp(offsets * offsets * (-0.5 / (sigma[:, None] * sigma[:, None])))
    return weights / weights.sum(axis=1, keepdims=True)


class BoxMaskGenerator(MaskGenerator):
    def __init__(self, prop_range, n_boxes=1, random_aspect_ratio=True, prop_by_area=True, within_bounds=True,
                 invert=False):
        if isinstance(prop_range, float):
            prop_range = (prop_range, prop_range)
        self.prop_range = prop_range
        self.n_boxes = n_boxes
        self.random_aspect_ratio = random_aspect_ratio
        self.prop_by_area = prop_by_area
        self.within_bounds = within_bounds
        self.invert = invert

    # ------------------------------------------------------------------ host: RNG draws (numpy call order kept)
    def generate_rectangles(self, n_masks, mask_shape, rng=None):
        """float64 (N, n_boxes, 4) rectangles [y0, x0, y1, x1] exactly as mask_gen.py:73-108 computes them."""
        if rng is None:
            rng = np.random
        lo, hi = self.prop_range
        nb = self.n_boxes
        dims = np.array(mask_shape)
        scale = np.sqrt(1.0 / nb)
        if self.prop_by_area:
            props = rng.uniform(lo, hi, size=(n_masks, nb))
            dead = props == 0.0
            if self.random_aspect_ratio:
                with np.errstate(divide='ignore', invalid='ignore'):
                    hy = np.exp(rng.uniform(low=0.0, high=1.0, size=(n_masks, nb)) * np.log(props))
                    wx = props / hy
                hy = hy * scale
                wx = wx * scale
            else:
                # the reference scales one shared array twice (mask_gen.py:84-87)
                hy = wx = np.sqrt(props) * scale * scale
            hy = np.where(dead, 0.0, hy)
            wx = np.where(dead, 0.0, wx)
        else:
            if self.random_aspect_ratio:
                hy = rng.uniform(lo, hi, size=(n_masks, nb)) * scale
                wx = rng.uniform(lo, hi, size=(n_masks, nb)) * scale
            else:
                hy = wx = rng.uniform(lo, hi, size=(n_masks, nb)) * scale * scale   # shared array, scaled twice
        sizes = np.round(np.stack([hy, wx], axis=2) * dims[None, None, :])
        if self.within_bounds:
            origin = np.round((dims - sizes) * rng.uniform(low=0.0, high=1.0, size=sizes.shape))
            return np.concatenate([origin, origin + sizes], axis=2)
        centre = np.round(dims * rng.uniform(low=0.0, high=1.0, size=sizes.shape))
        return np.concatenate([centre - sizes * 0.5, centre + sizes * 0.5], axis=2)

    @staticmethod
    def rectangles_to_ranges(rectangles, mask_shape):
        """numpy basic-slice rules of `m[int(y0):int(y1), int(x0):int(x1)]` -> int32 (N, nb, 4) [y0, y1, x0, x1]."""
        H, W = int(mask_shape[0]), int(mask_shape[1])
        flat = rectangles.reshape(-1, 4)
        out = np.empty((flat.shape[0], 4), dtype=np.int32)
        for i, (y0, x0, y1, x1) in enumerate(flat):
            ys, ye, _ = slice(int(y0), int(y1)).indices(H)
            xs, xe, _ = slice(int(x0), int(x1)).indices(W)
            out[i] = (ys, max(ys, ye), xs, max(xs, xe))
        return out.reshape(rectangles.shape[0], rectangles.shape[1], 4)

    def generate_ranges(self, n_masks, mask_shape, rng=None):
        """Device-path parameters: int32 (N, n_boxes, 4) numpy array."""
        return self.rectangles_to_ranges(self.generate_rectangles(n_masks, mask_shape, rng), mask_shape)

    # ------------------------------------------------------------------ reference-compatible surface
    def generate_params(self, n_masks, mask_shape, rng=None):
        """
        Box masks as a float64 `(N, 1, H, W)` numpy array, same values as the reference for the same `rng`
        (host-side, like the reference, which also builds them in DataLoader workers).
        """
        mask_shape = tuple(int(s) for s in mask_shape)
        ranges = self.generate_ranges(n_masks, mask_shape, rng)
        canvas = np.zeros((n_masks, 1) + mask_shape, dtype=bool)
        for i in range(n_masks):
            for ys, ye, xs, xe in ranges[i]:
                canvas[i, 0, ys:ye, xs:xe] ^= True
        if not self.invert:
            canvas = ~canvas
        return canvas.astype(np.float64)

    def torch_masks_from_params(self, t_params, mask_shape, torch_device):
        """
        Reference behaviour: identity on full masks (mask_gen.py:119-120). Device path: an int32 (N, nb, 4) range
        table is rasterised on the GPU.
        """
        if torch.is_tensor(t_params) and t_params.dtype == torch.int32 and t_params.dim() == 3 \
                and t_params.shape[-1] == 4:
            return ops.boxmask_rasterize(t_params.to(torch_device), mask_shape, self.invert)
        return t_params


class CowMaskGenerator(MaskGenerator):
    """
    CowMask (French, Oliver, Salimans, "Milking CowMask for semi-supervised image classification"): N(0,1) noise smoothed with a
    Gaussian of a random sigma and thresholded so that a random share p of the pixels is 1. The family that the reference's abstract
    `torch_masks_from_params` and its unused `gaussian_kernels` were scaffolding for; the reference itself has no such generator.

    Host draws, one RandomState, in this order: p = uniform(p_lo, p_hi, N); sigma = exp(uniform(log s_lo, log s_hi, N)). The noise
    is drawn on the device, and the blur, the statistics and the compare run there in fp64 (ops.cowmask, csrc/cowmask.hip):
        s = taps (*)_y (taps (*)_x noise), zero padded;  mask = [s <= mean(s) + std(s) * Phi^-1(p)]
    1 means "take image 1" in mix mode and "keep" in zero mode, like the default (inverted) box mask; there is no `invert`.
    """

    MAX_RADIUS = 128

    def __init__(self, prop_range, sigma_range, truncate=4.0):
        if isinstance(prop_range, (int, float)):
            prop_range = (float(prop_range), float(prop_range))
        if isinstance(sigma_range, (int, float)):
            sigma_range = (float(sigma_range), float(sigma_range))
        p_lo, p_hi = float(prop_range[0]), float(prop_range[1])
        s_lo, s_hi = float(sigma_range[0]), float(sigma_range[1])
        if not (0.0 <= p_lo <= p_hi <= 1.0):
            raise ValueError('CowMaskGenerator: prop_range {}:{} is not inside [0, 1]'.format(p_lo, p_hi))
        if not (s_lo > 0.0 and s_lo <= s_hi):
            raise ValueError('CowMaskGenerator: sigma_range {}:{} needs 0 < lo <= hi'.format(s_lo, s_hi))
        if not truncate > 0.0:
            raise ValueError('CowMaskGenerator: truncate must be positive')
        self.prop_range = (p_lo, p_hi)
        self.sigma_range = (s_lo, s_hi)
        self.truncate = float(truncate)
        self.radius = int(self.truncate * s_hi + 0.5)
        if self.radius > self.MAX_RADIUS:
            raise ValueError('CowMaskGenerator: sigma up to {} at truncate {} needs a radius of {}; at most {} is built'.format(
                s_hi, truncate, self.radius, self.MAX_RADIUS))

    # ------------------------------------------------------------------ host
    def generate_scalars(self, n_masks, rng=None):
        """(p, sigma), float64 (N,) each: the only host draws."""
        if rng is None:
            rng = np.random
        p = rng.uniform(self.prop_range[0], self.prop_range[1], size=(n_masks,))
        sigma = np.exp(rng.uniform(np.log(self.sigma_range[0]), np.log(self.sigma_range[1]), size=(n_masks,)))
        return p, sigma

    def generate_params(self, n_masks, mask_shape, rng=None):
        """float64 (N, 2) rows [p, sigma]: parameters on the host, masks from parameters on the device."""
        p, sigma = self.generate_scalars(n_masks, rng)
        return np.stack([p, sigma], axis=1)

    def kernel_table(self, sigma):
        """(taps float64 (N, 2R+1), R): every row as wide as the largest sigma of the RANGE asks for, normalised over that window"""
        return gaussian_kernels(sigma, max_sigma=self.sigma_range[1], truncate=self.truncate), self.radius

    @staticmethod
    def threshold_factors(p):
        """Phi^-1(p) in float64 (statistics.NormalDist); 0 at the end points p <= 0 and p >= 1, which are filled explicitly"""
        from statistics import NormalDist
        nd = NormalDist()
        return np.array([nd.inv_cdf(float(v)) if 0.0 < v < 1.0 else 0.0 for v in p], dtype=np.float64)

    # ------------------------------------------------------------------ device
    def torch_masks_from_params(self, t_params, mask_shape, torch_device, noise=None, generator=None):
        """(N, 2) [p, sigma] -> f32 (N,1,H,W) on `torch_device`. `noise`: f32 (N,1,H,W) standard normal; drawn with
        torch.randn(generator=generator) on the device when not given."""
        if torch.is_tensor(t_params):
            t_params = t_params.detach().cpu().numpy()
        params = np.asarray(t_params, dtype=np.float64)
        if params.ndim != 2 or params.shape[1] != 2:
            raise ValueError('CowMaskGenerator: params must be (N, 2) rows of [p, sigma], got {}'.format(params.shape))
        p, sigma = params[:, 0], params[:, 1]
        n, (H, W) = len(p), (int(mask_shape[0]), int(mask_shape[1]))
        if not (np.all(sigma > 0.0) and np.all(sigma <= self.sigma_range[1] * (1.0 + 1e-12))):
            raise ValueError('CowMaskGenerator: sigma outside (0, {}]'.format(self.sigma_range[1]))
        taps, _ = self.kernel_table(sigma)
        factors = self.threshold_factors(p)
        if noise is None:
            noise = torch.randn((n, 1, H, W), generator=generator, device=torch_device, dtype=torch.float32)
        elif tuple(noise.shape) != (n, 1, H, W):
            raise ValueError('CowMaskGenerator: noise has shape {}, {} expected'.format(tuple(noise.shape), (n, 1, H, W)))
        masks = ops.cowmask(noise, taps, factors)
        # the end points explicitly, not through infinite thresholds
        for i in np.nonzero(p <= 0.0)[0]:
            masks[int(i)].zero_()
        for i in np.nonzero(p >= 1.0)[0]:
            masks[int(i)].fill_(1.0)
        return masks


class ClassMixGenerator(MaskGenerator):
    """
    ClassMix (Olsson, Tranheden, Pinto, Svensson, "ClassMix: Segmentation-Based Data Augmentation for Semi-Supervised Learning",
    WACV 2021): the mask of a sample is the region that the teacher predicts, on image 1, to belong to a random half of the classes
    it predicts there. Not in the reference. 1 means "take image 1", like the default (inverted) box mask; there is no `invert`.

    Host draw, one RandomState, ONE call per batch: keys = rng.random_sample((N, n_classes)), row n for sample n. Everything else
    runs on the device (ops.classmix_mask, csrc/classmix.hip): the full-resolution argmax of the teacher's low-resolution logits,
    the set of classes present among the sample's valid pixels, and of its m classes the k = (m + 1) // 2 with the smallest (key,
    class index) -- a uniformly random subset of that size, since the keys are i.i.d. k = ceil(m / 2) is the rule of the authors'
    published code as far as we recall it; it has not been tuned here.

    `needs_teacher` tells train_seg_semisup_mask_mt.mask_mt_job to make the mask after the unsupervised images are staged, from the
    teacher's logits of image 1 (`torch_masks_from_logits`); there is no `generate_ranges`, so the step takes a materialised mask.
    """

    needs_teacher = True

    def generate_params(self, n_masks, n_classes, rng=None):
        """float64 (N, n_classes) keys, uniform on [0, 1): the only host draw"""
        if rng is None:
            rng = np.random
        return rng.random_sample((int(n_masks), int(n_classes)))

    def torch_masks_from_logits(self, keys, logits, out_size, align_corners, valid=None):
        """keys (N, C) from generate_params, logits (N, C, h, w) on the device, valid optional f32 (N,1,H,W) -> f32 (N,1,H,W)"""
        return ops.classmix_mask(logits, keys, out_size, align_corners=align_corners, valid=valid)


class AddMaskParamsToBatch(object):
    """
    Collate hook (mask_gen.py:123-142): adds `mask_params` to every sample of a batch. With `as_ranges=True` the
    per-sample entry is the (n_boxes, 4) int32 range table instead of a full-resolution fp32 mask, which removes the
    N*H*W*4-byte host->device copy per iteration.
    """

    def __init__(self, mask_gen, as_ranges=False):
        self.mask_gen = mask_gen
        self.as_ranges = as_ranges

    def __call__(self, batch):
        sample = batch[0]
        sample0 = sample['sample0'] if 'sample0' in sample else sample
        mask_size = sample0['image'].shape[1:3]
        if self.as_ranges:
            params = self.mask_gen.generate_ranges(len(batch), mask_size)
            for sample, p in zip(batch, params):
                sample['mask_params'] = p
        else:
            params = self.mask_gen.generate_params(len(batch), mask_size)
            for sample, p in zip(batch, params):
                sample['mask_params'] = p.astype(np.float32)
        return batch
