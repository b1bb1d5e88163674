"""Test helper shared by tests/test_pair_stage_cpu.py and tests/test_gpu_pair_stage.py: the pair configurations with their seeds,
the map output pixel -> source position a parameter row implies, the ramp sources, one view staged by oracle/augment.py from a
row (the mask mode included), and the reference's own debugging check of a pair (train_seg_semisup_aug_mt.py:315-338: warp view 0
into view 1 with xf0_to_1 and compare where both masks are 1)."""
import numpy as np

N_PAIRS, SEED = 40, 5
# name -> (crop, source size, PairGeometry options): self-consistency of N_PAIRS pairs each, drawn from RandomState(SEED)
SELF_CONSISTENCY = {
    'plain': ((33, 41), (60, 70), dict()),
    'flips': ((33, 41), (60, 70), dict(hflip=True, vflip=True)),
    'transpose': ((33, 33), (60, 70), dict(hflip=True, vflip=True, hvflip=True)),
    'hung': ((33, 41), (60, 70), dict(scale_hung=True)),
    'hung_padded': ((33, 41), (37, 53), dict(scale_hung=True, hflip=True)),
    'hung_nonuniform': ((33, 41), (60, 70), dict(scale_hung=True, scale_non_uniform=True)),
    'warp30_scale1.5': ((33, 41), (60, 70), dict(rot_mag=30.0, max_scale=1.5, hflip=True)),
    'free_scale_rot': ((33, 41), (60, 70), dict(rot_mag=30.0, max_scale=1.5, free_scale_rot=True)),
    'warp_small_source': ((33, 41), (20, 90), dict(rot_mag=30.0, max_scale=1.5)),
}
MAX_LEVELS = 1.5           # grey levels: 0.5 quantisation per view + 0.5 floating-point margin (see compare_views)
MIN_COMPARED = 0.10        # every pair compares at least this share of its pixels

# name -> (crop, PairGeometry options, augmenter options, rng seed, colour seed): pairs over the ragged pool of _stage_cases
# (INDEX: 8 samples, entries from 1 x 1 to 90 x 20), staged view by view against the oracle
RAGGED = {
    'plain': ((48, 64), dict(), dict(), 1, 101),
    'flips_transpose': ((48, 48), dict(hflip=True, vflip=True, hvflip=True), dict(), 1, 101),
    'hung': ((48, 64), dict(scale_hung=True, hflip=True), dict(), 1, 101),
    'hung_nonuniform': ((48, 64), dict(scale_hung=True, scale_non_uniform=True), dict(), 1, 101),
    'warp30_scale1.5': ((48, 64), dict(rot_mag=30.0, max_scale=1.5, vflip=True), dict(), 1, 101),
    'free_scale_rot': ((48, 64), dict(rot_mag=30.0, max_scale=1.5, free_scale_rot=True, scale_non_uniform=True), dict(), 1, 101),
    'hung_strong_colour': ((48, 64), dict(scale_hung=True, hflip=True), dict(strong_colour=True), 1, 101),
}


def make_geometry(crop, cfg, seed):
    from cutmix_semisup_seg_amd.aug_pairs import PairGeometry
    return PairGeometry(crop, rng=np.random.RandomState(seed), **cfg)


def row_source_position(p, crop, ox, oy):
    """Source position (sx, sy), in float64, that the staging kernel samples for output pixel (ox, oy) of a row: the un-flip
    (transpose, y flip, x flip: stage_unflip), then the window map (c + 0.5) * sc / crop - 0.5 + origin or the warp of slots
    16..21."""
    H, W = crop
    cx, cy = float(ox), float(oy)
    if p[6]:
        cx, cy = cy, cx
    if p[5]:
        cy = H - 1 - cy
    if p[4]:
        cx = W - 1 - cx
    a = np.asarray(p, dtype=np.float64)
    if p[15]:
        return a[16] * cx + a[17] * cy + a[18], a[19] * cx + a[20] * cy + a[21]
    return (cx + 0.5) * a[3] / W - 0.5 + a[1], (cy + 0.5) * a[2] / H - 0.5 + a[0]


def assert_pair_branches_covered(cfg, params, crop):
    """Every configured branch occurs in the rows of the batch (what _stage_cases.assert_branches_covered asserts for single
    views); params (2, n, 24)."""
    for slot, opt in ((4, 'hflip'), (5, 'vflip'), (6, 'hvflip')):
        for v in range(2):
            if cfg.get(opt):
                assert set(params[v, :, slot].tolist()) == {0.0, 1.0}, (opt, v, params[v, :, slot])
            else:
                assert not params[v, :, slot].any()
    if cfg.get('rot_mag') and not cfg.get('scale_hung'):
        assert (params[:, :, 15] == 1).all() and (params[:, :, 22] == 1).all() and not params[:, :, 23].any()
        same = np.isclose(params[0, :, 16:18], params[1, :, 16:18]).all(axis=1)
        assert not same.any() if cfg.get('free_scale_rot') else same.all()      # one (scale, angle) per view, or one per pair
    else:
        assert not params[:, :, 15].any()
    assert (params[0, :, 2:4] == crop).all() and not params[0, :, 23].any()     # view 0 is never resized
    if cfg.get('scale_hung'):
        assert (params[1, :, 23] == 1).all()
        sizes = {tuple(r) for r in params[1, :, 2:4].tolist()}
        assert len(sizes) > 1 and any(s[0] > crop[0] for s in sizes) and any(s[0] < crop[0] for s in sizes)
        if cfg.get('scale_non_uniform'):
            assert any(abs(r[0] * crop[1] - r[1] * crop[0]) > crop[0] for r in params[1, :, 2:4])
    else:
        assert not params[1, :, 23].any()
        if not cfg.get('rot_mag'):
            assert (params[1, :, 2:4] == crop).all()


def ramp_source(size_hw):
    """uint8 ramps affine in (x, y), one slope per channel, 255 / (longest side - 1) grey levels per pixel: along x, along y, and
    falling along the diagonal. Bilinear sampling of the un-rounded ramp is exact; rounding to uint8 moves each pixel <= 0.5."""
    h, w = size_hw
    s = 255.0 / (max(h, w) - 1)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    return np.round(np.stack([s * xx, s * yy, 255.0 - s * 0.5 * (xx + yy)], axis=2)).astype(np.uint8)


def oracle_view(src, row, crop, mean, std, pivot=None):
    """One view staged by oracle/augment.py from its row -> (image (3,H,W), colour image (3,H,W), mask (H,W)). Mask mode 1 (slot
    23) is the oracle's nearest in-bounds test: where the label it reads from an all-zero label map is not 255."""
    from oracle import augment as oaug
    lab = np.zeros(src.shape[:2], dtype=np.uint8) if row[23] else None
    i0, i1, lb, alpha = oaug.augment_sample(src, lab, row, crop, mean, std, pivot=pivot)
    return i0, i1, ((lb != 255).astype(np.float64) if row[23] else alpha)


def compare_views(image0, image1, mask0, mask1, xf0_to_1):
    """The reference's debugging check for a batch of pairs. image* (n,3,H,W) in [0, 1] (staged with mean 0, std 1), mask*
    (n,1,H,W), xf0_to_1 (n,2,3); torch tensors on one device. View 0 and its mask are warped into view 1 with
    F.affine_grid / F.grid_sample(align_corners=True) and compared with view 1 where the warped mask and view 1's mask are both 1
    (to 1e-5, the mask tolerance of _stage_cases).
    -> per pair: (largest difference in grey levels, share of the pixels compared).

    Why MAX_LEVELS = 1.5: bilinear sampling of an affine image is exact, so each view carries at most the 0.5 level of the source's
    quantisation; grid_sample is a convex combination and adds none, so the views differ by at most 1.0 level, + 0.5 for floating
    point. A misalignment of half a pixel at the ramps' 2.9 - 4.9 levels per pixel fails it."""
    import torch
    import torch.nn.functional as F
    theta = torch.as_tensor(xf0_to_1, dtype=torch.float32, device=image0.device)
    grid = F.affine_grid(theta, list(image0.shape), align_corners=True)
    x0_in_1 = F.grid_sample(image0.float(), grid, align_corners=True)
    m0_in_1 = F.grid_sample(mask0.float(), grid, align_corners=True)
    both = (m0_in_1 >= 1.0 - 1e-5) & (mask1.float() >= 1.0 - 1e-5)
    diff = (x0_in_1 - image1.float()).abs().amax(dim=1, keepdim=True) * 255.0
    worst = torch.where(both, diff, torch.zeros_like(diff)).flatten(1).amax(dim=1)
    share = both.float().flatten(1).mean(dim=1)
    return worst.cpu().numpy(), share.cpu().numpy()
