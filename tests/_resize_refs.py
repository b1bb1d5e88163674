"""The ISIC 2017 converter's area resize and statistics restated in numpy, in our own words: what tests/test_resize_cpu.py holds
csrc/resize_math.hpp to on the host and tests/test_gpu_resize.py holds the kernels and the converter to on the device.

    weight_matrix    (Lo, L) int64: in units of 1 / Lo pixel, pixel i covers [i Lo, (i + 1) Lo), cell o covers [o L, (o + 1) L);
                     the entry is the length of their overlap
    numerators       sum_iy sum_ix wy wx p, int64, by two einsum contractions
    area_resize_u8   numerators / (h w), rounded to nearest, an exact half to the even neighbour
    mean_std         the reference's float64 statistics (convert_isic.py:67-73) of a list of uint8 images
"""
import numpy as np


def weight_matrix(L, Lo):
    assert 1 <= Lo <= L
    o, i = np.arange(Lo, dtype=np.int64)[:, None], np.arange(L, dtype=np.int64)[None, :]
    return np.clip(np.minimum((i + 1) * Lo, (o + 1) * L) - np.maximum(i * Lo, o * L), 0, None)


def numerators(x, ho, wo):
    """x uint8 (N, H, W, C) or (N, H, W) -> int64 (N, ho, wo, C) or (N, ho, wo)"""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim in (3, 4)
    x4 = (x if x.ndim == 4 else x[..., None]).astype(np.int64)
    wy, wx = weight_matrix(x4.shape[1], ho), weight_matrix(x4.shape[2], wo)
    rows = np.einsum('oi,nijc->nojc', wy, x4, optimize=True)
    num = np.einsum('pj,nojc->nopc', wx, rows, optimize=True)
    return num if x.ndim == 4 else num[..., 0]


def round_half_even_div(num, den):
    q, r = np.divmod(np.asarray(num, dtype=np.int64), np.int64(den))
    return q + ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))


def area_resize_u8(x, ho, wo):
    x = np.asarray(x)
    out = round_half_even_div(numerators(x, ho, wo), x.shape[1] * x.shape[2])
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def is_tie(x, ho, wo):
    """where the quotient is an exact half"""
    x = np.asarray(x)
    den = x.shape[1] * x.shape[2]
    return 2 * (numerators(x, ho, wo) % den) == den


def sum_sumsq(x):
    """x uint8 (N, H, W, C) or (N, H, W) -> int64 (N, 2C): sum p per channel, then sum p^2"""
    x = np.asarray(x)
    x4 = (x if x.ndim == 4 else x[..., None]).astype(np.int64)
    return np.concatenate([x4.sum(axis=(1, 2)), (x4 * x4).sum(axis=(1, 2))], axis=1)


def mean_std(images):
    """The reference's accumulation over uint8 (H, W, 3) images: img_as_float is p / 255 in float64"""
    rgb_sum, rgb2_sum, rgb_n = np.zeros((3,)), np.zeros((3,)), 0
    for img in images:
        rgb = np.asarray(img).astype(np.float64) / 255.0
        rgb_sum += rgb.sum(axis=(0, 1))
        rgb2_sum += (rgb ** 2).sum(axis=(0, 1))
        rgb_n += rgb.shape[0] * rgb.shape[1]
    return rgb_sum / rgb_n, np.sqrt(rgb2_sum / rgb_n - rgb_sum * rgb_sum / rgb_n / rgb_n)


# (n, h, w, c, ho, wo): degenerate and identity; factor 2; fractional overlap on both axes for c = 3 and c = 1; a factor just above 1;
# the whole image into one cell; more source columns than a workgroup has threads, and a tall narrow source; the real target width
# with several column segments and an odd row pitch; the widest ISIC row
SMALL_CASES = [(1, 1, 1, 3, 1, 1), (1, 5, 7, 3, 5, 7), (2, 4, 6, 3, 2, 3), (2, 7, 10, 3, 3, 4), (1, 10, 14, 1, 4, 4), (1, 9, 9, 1, 8, 8),
               (1, 64, 64, 3, 1, 1), (1, 3, 300, 3, 2, 7), (1, 300, 3, 1, 7, 2), (1, 37, 1030, 3, 5, 248), (1, 20, 6748, 3, 2, 248)]
FRAME_CASE = (1, 767, 1022, 3, 248, 248)                       # one real-size frame
BIG_NUMERATOR_CASE = (1, 4160, 4160, 1, 2, 3)                  # numerators above 2^32


def case_id(case):
    return 'x'.join(map(str, case))


_INPUTS, _WANT = {}, {}


def case_inputs(case):
    """-> {name: uint8 source}, the same arrays on every call (they are shared: do not write to them)"""
    if case not in _INPUTS:
        n, h, w, c, ho, wo = case
        shape = (n, h, w, 3) if c == 3 else (n, h, w)
        rng = np.random.RandomState(sum(case))
        if case == FRAME_CASE:
            inputs = dict(noise=rng.randint(0, 256, size=shape).astype(np.uint8))
        elif case == BIG_NUMERATOR_CASE:
            inputs = dict(bright=rng.randint(250, 256, size=shape).astype(np.uint8), white=np.full(shape, 255, dtype=np.uint8))
        else:
            inputs = dict(noise=rng.randint(0, 256, size=shape).astype(np.uint8), white=np.full(shape, 255, dtype=np.uint8))
            if c == 3:
                inputs['channels'] = np.broadcast_to(np.array([11, 130, 251], dtype=np.uint8), shape).copy()
            else:
                inputs['binary'] = (rng.randint(0, 2, size=shape) * 255).astype(np.uint8)
            if case == (2, 4, 6, 3, 2, 3):
                inputs['ties'] = tie_image(rng)[0]
        _INPUTS[case] = inputs
    return _INPUTS[case]


def case_want(case, name):
    """the restatement's output for an input of case_inputs, computed once"""
    if (case, name) not in _WANT:
        _WANT[case, name] = area_resize_u8(case_inputs(case)[name], case[4], case[5])
    return _WANT[case, name]


def tie_image(rng, n=2, ho=2, wo=3):
    """(n, 2 ho, 2 wo, 3) of 2 x 2 blocks [k, k, k + 1, k + 1] with random k: at factor 2 every output is k + 1/2, an exact half, and
    ties-to-even gives k + k % 2 -> (image, k (n, ho, wo, 3))"""
    k = rng.randint(0, 255, size=(n, ho, 1, wo, 1, 3))
    bump = np.array([[0, 0], [1, 1]])
    x = k + bump[None, None, :, None, :, None]
    return x.reshape(n, 2 * ho, 2 * wo, 3).astype(np.uint8), k.reshape(n, ho, wo, 3)
