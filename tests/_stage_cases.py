"""Test helper shared by tests/test_stage_hostcheck.py (CPU) and tests/test_gpu_stage.py: the ragged pool, the batch index, the
staging configurations with their seeds, and the per-sample comparison with oracle/augment.py."""
import numpy as np

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
# smaller than the crop in one axis and in both, equal to it, one pixel (reflect101 with n == 1), rows at odd byte offsets
POOL_SIZES = [(37, 53), (60, 70), (48, 64), (20, 90), (90, 20), (5, 3), (1, 1)]
INDEX = [6, 0, 3, 3, 1, 5, 2, 4]                 # an entry used twice, out of order
# name -> (crop, with_labels, DeviceAugmenter options, rng seed, colour seed)
CONFIGS = {
    'plain_crop': ((48, 64), True, dict(), 1, 101),
    'hung_flips': ((48, 48), True, dict(scale_hung=True, hflip=True, vflip=True, hvflip=True), 1, 101),
    'hung_nonuniform': ((48, 64), True, dict(scale_hung=True, scale_non_uniform=True), 1, 101),
    'rot30_scale1.5_sup': ((48, 64), True, dict(rot_mag=30.0, max_scale=1.5), 1, 101),
    'rot30_scale1.5_unsup': ((48, 64), False, dict(rot_mag=30.0, max_scale=1.5), 1, 101),
    'colour': ((48, 64), False, dict(strong_colour=True, scale_hung=True, hflip=True), 1, 101),
}


def make_pool_arrays(seed=7):
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in POOL_SIZES]
    labels = [rng.randint(0, 5, size=(h, w)).astype(np.uint8) for h, w in POOL_SIZES]
    return images, labels


def make_augmenter(name, out_dtype=None):
    import torch
    from cutmix_semisup_seg_amd.device_pipeline import DeviceAugmenter
    crop, with_labels, cfg, seed, cseed = CONFIGS[name]
    aug = DeviceAugmenter(crop, MEAN, STD, out_dtype=out_dtype or torch.float32, rng=np.random.RandomState(seed),
                          colour_rng=np.random.RandomState(cseed), **cfg)
    return aug, crop, with_labels, cfg


def assert_branches_covered(name, params):
    """Every configured branch occurs in the rows of the batch."""
    _, _, cfg, _, _ = CONFIGS[name]
    for slot, opt in ((4, 'hflip'), (5, 'vflip'), (6, 'hvflip')):
        if cfg.get(opt):
            assert set(params[:, slot].tolist()) == {0.0, 1.0}, (opt, params[:, slot])
        else:
            assert not params[:, slot].any()
    if cfg.get('rot_mag'):
        assert (params[:, 15] == 1).all()
        want = {0.0} if CONFIGS[name][1] else {0.0, 1.0}           # labelled: nearest; otherwise both interpolation modes
        assert set(params[:, 22].tolist()) == want
    else:
        assert not params[:, 15].any()
    if cfg.get('scale_hung'):
        assert len({tuple(r) for r in params[:, 2:4].tolist()}) > 1           # different window sizes (scales)
        if cfg.get('scale_non_uniform'):
            crop = CONFIGS[name][0]
            assert any(abs(r[0] * crop[1] - r[1] * crop[0]) > crop[0] for r in params[:, 2:4])   # aspect differs from the crop's
    if cfg.get('strong_colour'):
        assert set(params[:, 12].tolist()) == {0.0, 1.0}            # jitter applied and not applied
        assert params[:, 11].any()                                  # greyscale drawn at least once


def oracle_pivot(src, p, crop):
    """The contrast pivot the device computes: mean luminance of the geometric transform (x brightness where it comes first)."""
    from oracle import augment as oaug
    geo_only = np.ones(p.shape[0])
    geo_only[10:15] = 0
    img0, _, _, _ = oaug.augment_sample(src, None, p * geo_only, crop, np.zeros(3), np.ones(3))
    luma = float((img0.transpose(1, 2, 0) @ oaug.GREY).mean())
    order = int(p[13])
    ops_ = [(order >> s) & 3 for s in (6, 4, 2, 0)]
    return luma * (p[7] if ops_.index(0) < ops_.index(1) else 1.0)


ROUNDING_MARGIN = 1e-4     # source pixels; see near_rounding_boundary
MAX_BOUNDARY_FRACTION = 2e-3


def near_rounding_boundary(p, crop):
    """Warp rows with NEAREST interpolation round the source coordinate of every output pixel, floor(s + 0.5). The kernel
    evaluates s = a x + b y + c in fp32 (two fused multiply-adds; |s| stays below a few hundred pixels here, where fp32 is
    spaced 1.5e-5 .. 3e-5 apart, so its error is below 1e-4), the oracle in float64: a pixel whose exact coordinate lies within
    1e-4 of k + 0.5 may legitimately land on the neighbouring source pixel (tests/test_gpu_augment.py's docstring states the same
    figure; cv2's own 1/1024 fixed point moves far more). -> (H, W) bool map of those pixels in OUTPUT orientation, None for rows
    that do not round (window mode, bilinear warps: both are continuous across the boundary)."""
    from oracle import augment as oaug
    if not p[15] or p[22]:
        return None
    H, W = crop
    a = np.asarray(p[16:22], dtype=np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    near = np.zeros((H, W), dtype=bool)
    for s in (a[0] * xx + a[1] * yy + a[2], a[3] * xx + a[4] * yy + a[5]):
        f = s + 0.5
        near |= np.abs(f - np.round(f)) < ROUNDING_MARGIN
    return oaug._flip(near, bool(p[4]), bool(p[5]), bool(p[6]))


def compare_with_oracle(name, params, images, labels, out):
    """out: dict of numpy arrays image (N,3,H,W), mask (N,H,W), labels (N,H,W) | None, image_stu (N,3,H,W) | None. Every sample
    of the batch is compared: image 2e-4, mask 1e-5, labels exact, colour view 2e-3 (tests/test_gpu_augment.py's bounds). In
    rows that round source coordinates, the pixels within ROUNDING_MARGIN of a rounding boundary are set aside; there may be at
    most MAX_BOUNDARY_FRACTION of them in the batch (the bound tests/test_gpu_augment.py puts on such pixels).
    -> the largest differences seen (image, mask, colour)"""
    from oracle import augment as oaug
    crop, with_labels, cfg, _, _ = CONFIGS[name]
    worst = [0.0, 0.0, 0.0]
    set_aside = total = 0
    for i, e in enumerate(INDEX):
        src, lab = images[e], (labels[e] if with_labels else None)
        pivot = oracle_pivot(src, params[i], crop) if (cfg.get('strong_colour') and params[i, 12]) else None
        i0, i1, lb, al = oaug.augment_sample(src, lab, params[i], crop, MEAN, STD, pivot=pivot)
        near = near_rounding_boundary(params[i], crop)
        keep = np.ones(crop, dtype=bool) if near is None else ~near
        set_aside += int((~keep).sum())
        total += keep.size
        worst[0] = max(worst[0], float(np.abs(out['image'][i] - i0)[:, keep].max()))
        worst[1] = max(worst[1], float(np.abs(out['mask'][i] - al)[keep].max()))
        np.testing.assert_allclose(out['image'][i][:, keep], i0[:, keep], rtol=2e-4, atol=2e-4, err_msg='image, sample {}'.format(i))
        np.testing.assert_allclose(out['mask'][i][keep], al[keep], rtol=1e-5, atol=1e-5, err_msg='mask, sample {}'.format(i))
        if with_labels:
            assert np.array_equal(out['labels'][i][keep], lb[keep]), 'labels, sample {}'.format(i)
        if cfg.get('strong_colour'):
            worst[2] = max(worst[2], float(np.abs(out['image_stu'][i] - i1)[:, keep].max()))
            np.testing.assert_allclose(out['image_stu'][i][:, keep], i1[:, keep], rtol=2e-3, atol=2e-3,
                                       err_msg='colour view, sample {}'.format(i))
    assert set_aside <= MAX_BOUNDARY_FRACTION * total, (set_aside, total)
    return worst
