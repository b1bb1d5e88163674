"""
Writes tests/golden/patch_dist.npz from the reference's own patch_dist.py (needs scipy for its fftconvolve):

    python tests/golden/make_patch_dist_golden.py PATH_TO_THE_REFERENCE_CHECKOUT

Data only: seeded label maps (with void 255s) and what the reference's neighbouring_pixels_class_change / boundary_pixels make of
them; two small seeded uint8 images with patches, and the reference's sliding_window_distance_to_patches_generator maps on
img_as_float's view of them (uint8 / 255). `*_ref_err` is the reference's own error: the largest |golden^2 - exact^2| over the
fixture, exact being the int64 brute force (tests/_patch_dist_refs.py) over 255^2 -- the tests allow ten times that.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _patch_dist_refs as R          # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location('reference_patch_dist', os.path.join(root, 'patch_dist.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def label_map(rng, h, w, n_classes):
    """blocky classes with void specks: boundaries, void next to boundaries, void on the border"""
    lab = rng.randint(0, n_classes, size=(h // 3 + 1, w // 3 + 1)).repeat(3, 0).repeat(3, 1)[:h, :w].astype(np.uint8)
    lab[rng.uniform(size=(h, w)) < 0.08] = 255
    lab[0, 0] = lab[h - 1, w // 2] = 255
    return lab


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.RandomState(20240)
    out = {}
    for name, (h, w, c) in (('lab_a', (17, 23, 4)), ('lab_b', (9, 12, 2)), ('lab_c', (3, 3, 3))):
        lab = label_map(rng, h, w, c)
        out[name] = lab
        out[name + '_change'] = np.stack(ref.neighbouring_pixels_class_change(lab))
        out[name + '_boundary'] = ref.boundary_pixels(lab)
    for name, (h, w), shape, n in (('img_a', (23, 31), (7, 7), 3), ('img_b', (6, 19), (9, 5), 2)):
        image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        other = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        # one patch cut from the image itself (a true distance of 0 somewhere), the others from elsewhere
        centres = [(h // 2, w // 2)] + [(int(rng.randint(0, h)), int(rng.randint(0, w))) for _ in range(n - 1)]
        patches = np.stack([R.cut_patch(image if k == 0 else other, shape, yx) for k, yx in enumerate(centres)]).astype(np.uint8)
        maps = np.stack(list(ref.sliding_window_distance_to_patches_generator(image / 255.0, patches / 255.0)))
        exact = R.brute_d2(image, patches).astype(np.float64) / 255.0 ** 2
        out[name], out[name + '_patches'], out[name + '_maps'] = image, patches, maps
        out[name + '_ref_err'] = np.array(np.abs(maps ** 2 - exact).max())
        print(name, 'reference error on squared distances:', float(out[name + '_ref_err']), 'max', float(exact.max()))
    np.savez_compressed(os.path.join(HERE, 'patch_dist.npz'), **out)


if __name__ == '__main__':
    main()
