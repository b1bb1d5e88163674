"""The arithmetic of the reference's Cityscapes converter restated in numpy, in our own words: what tests/test_convert_cpu.py holds
csrc/convert_math.hpp to on the host and tests/test_gpu_convert.py holds the kernels to on the device.

    block_mean_u8   the float64 mean of each d x d block of an (H, W, 3) or (N, H, W, 3) uint8 image, truncated by astype(uint8)
                    (what skimage's downscale_local_mean(x, (d, d, 1)).astype(np.uint8) computes)
    block_vote      a one-hot count of every value over each d x d block of an (H, W) or (N, H, W) map, then argmax: the most
                    frequent value, the lowest among equally frequent ones
"""
import numpy as np


def block_mean_u8(x, d):
    x = np.asarray(x)
    lead = x.shape[:-3]
    h, w, c = x.shape[-3:]
    assert h % d == 0 and w % d == 0
    blocks = x.reshape(lead + (h // d, d, w // d, d, c)).astype(np.float64)
    return blocks.mean(axis=(-4, -2)).astype(np.uint8)


def block_vote(y, d):
    y = np.asarray(y)
    lead = y.shape[:-2]
    h, w = y.shape[-2:]
    assert h % d == 0 and w % d == 0
    n_values = int(y.max()) + 1
    blocks = y.reshape(lead + (h // d, d, w // d, d))
    counts = np.zeros(lead + (h // d, w // d, n_values), dtype=np.int64)
    for v in range(n_values):                                  # one plane of the one-hot array at a time
        counts[..., v] = (blocks == v).sum(axis=(-3, -1))
    return np.argmax(counts, axis=-1).astype(np.uint8)


def hand_made_ties():
    """2 x 2 blocks in every arrangement of counts, with the winner counted by hand and the lowest value in every position
    -> (labels (1, 2, 2 * B), winners (1, 1, B))"""
    blocks = [[7, 7, 7, 7], [9, 3, 3, 9], [3, 9, 9, 3], [200, 5, 5, 200], [1, 2, 3, 4], [4, 3, 2, 1], [2, 4, 1, 3], [255, 0, 255, 0],
              [0, 255, 0, 255], [6, 6, 2, 9], [2, 9, 6, 6], [9, 2, 2, 2], [254, 255, 255, 254], [33, 0, 33, 0], [5, 5, 5, 1],
              [8, 1, 1, 8], [0, 0, 1, 1], [1, 1, 0, 0], [1, 0, 1, 0], [17, 18, 18, 19]]
    want = [7, 3, 3, 5, 1, 1, 1, 0, 0, 6, 6, 2, 254, 0, 5, 1, 0, 0, 0, 18]
    y = np.array(blocks, dtype=np.uint8).reshape(len(blocks), 2, 2).transpose(1, 0, 2).reshape(1, 2, 2 * len(blocks))
    return y, np.array(want, dtype=np.uint8).reshape(1, 1, len(blocks))


def distinct_blocks(rng, n_blocks=6):
    """8 x 8 blocks of 64 distinct values each -> (labels (1, 8, 8 * n_blocks), the smallest value of each block)"""
    blocks = [rng.permutation(256)[:64] for _ in range(n_blocks)]
    y = np.stack([b.reshape(8, 8) for b in blocks], axis=1).reshape(1, 8, 8 * n_blocks).astype(np.uint8)
    return y, np.array([b.min() for b in blocks], dtype=np.uint8).reshape(1, 1, n_blocks)


def floor_not_round_image(rng, n, h, w, d):
    """An image whose every block sum is -1 mod d^2 (d^2 - 1 cells one above the block's base value): rounding to nearest would
    give base + 1 where truncation gives base"""
    base = rng.randint(0, 255, size=(n, h // d, 1, w // d, 1, 3))
    bump = np.ones((d, d), dtype=np.int64)
    bump[rng.randint(0, d), rng.randint(0, d)] = 0
    x = base + bump[None, None, :, None, :, None]
    return x.reshape(n, h, w, 3).astype(np.uint8), base.reshape(n, h // d, w // d, 3).astype(np.uint8)


def sums_image(d):
    """An image (d, d * (255 d^2 + 1), 3) whose block s has the sum s in every channel: every possible block sum once"""
    n = 255 * d * d + 1
    s = np.arange(n)
    q, r = s // (d * d), s % (d * d)
    cells = q[:, None] + (np.arange(d * d)[None, :] < r[:, None])             # r cells of q + 1, the rest q
    assert cells.max() <= 255 and np.array_equal(cells.sum(1), s)
    img = cells.reshape(n, d, d).transpose(1, 0, 2).reshape(d, n * d)
    return np.repeat(img[:, :, None], 3, axis=2).astype(np.uint8)
