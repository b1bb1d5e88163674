"""
Writes tests/golden/neighbour_dist.npz from the reference's own patch_dist.py (which imports scipy):

    python tests/golden/make_neighbour_dist_golden.py PATH_TO_THE_REFERENCE_CHECKOUT

Data only: three seeded uint8 images, and for each (image, patch size) case the reference's neighbouring_patch_distance_maps (the
four maps stacked: left, right, up, down) and patch_average_distance_map on img_as_float's view of the image (uint8 / 255); its
box_sum of a seeded float plane and of an integer plane. `*_ref_err` is the reference's own error per case: the largest
|g^2 * 65025 - D2| over its finite values, D2 being the int64 brute force (tests/_neighbour_dist_refs.py).

The reference sums img_as_float values in a float64 summed-area table, which cancels to about +-1e-13 where the true sum is 0;
np.sqrt makes NaN of the negative ones. That happens on flat regions that follow textured ones, which is what `img_c` is. The
script asserts that the noise images give no NaN, that every NaN of img_c sits where the exact D2 is 0, and that img_c has more
exact zeros than NaNs (so the tests see zeros of both kinds).
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _neighbour_dist_refs as R          # noqa: E402

CASES = (('img_a', ((3, 3), (5, 3), (15, 15))), ('img_b', ((7, 7),)), ('img_c', ((5, 5),)))


def load_reference(root):
    spec = importlib.util.spec_from_file_location('reference_patch_dist', os.path.join(root, 'patch_dist.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_key(name, shape):
    return '{}_p{}x{}'.format(name, shape[0], shape[1])


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.RandomState(20241)
    out = {}
    out['img_a'] = rng.randint(0, 256, size=(12, 5, 3)).astype(np.uint8)
    out['img_b'] = rng.randint(0, 256, size=(20, 26, 3)).astype(np.uint8)
    img_c = rng.randint(0, 256, size=(24, 31, 3)).astype(np.uint8)
    img_c[12:, 15:] = 131                                     # the lower-right quadrant: one grey level after texture
    out['img_c'] = img_c
    for name, shapes in CASES:
        image = out[name]
        for shape in shapes:
            key = case_key(name, shape)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)           # np.sqrt of the cancelled sums
                maps = np.stack(ref.neighbouring_patch_distance_maps(image / 255.0, shape))
                avg = ref.patch_average_distance_map(image / 255.0, shape)
            d2 = R.brute_neighbour_d2(image, shape)
            nans, zeros = int(np.isnan(maps).sum()), int((d2 == 0).sum())
            ok, err = R.golden_agrees(maps, d2)
            assert ok, key
            assert maps.shape == d2.shape and avg.shape == d2.shape[1:]
            if name == 'img_c':
                assert (d2[np.isnan(maps)] == 0).all() and nans < zeros, (key, nans, zeros)
            else:
                assert nans == 0, (key, nans)
            out[key + '_maps'], out[key + '_avg'], out[key + '_ref_err'] = maps, avg, np.array(err)
            print(key, 'NaNs', nans, 'exact zeros', zeros, 'reference error |g^2 * 65025 - D2|:', err, 'max D2', int(d2.max()))
    out['box_float_plane'] = rng.uniform(size=(11, 14))
    out['box_float_sum'] = ref.box_sum(out['box_float_plane'], (3, 5))
    out['box_int_plane'] = rng.randint(0, 3 * 255 * 255 + 1, size=(9, 13)).astype(np.int64)
    out['box_int_sum'] = ref.box_sum(out['box_int_plane'], (5, 3))
    assert out['box_int_sum'].dtype == np.int64
    path = os.path.join(HERE, 'neighbour_dist.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
