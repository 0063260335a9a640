"""Inputs and shapes shared by tests/test_ssim_cpu.py and tests/test_gpu_ssim.py."""
import numpy as np


def pair(shape, seed, rows=None, texture=0.2):
    """x (B, C, H, W) and y ((R,) B, C, H, W) as float32 in [-1, 1]: a blocky random picture under uniform noise of amplitude `texture` and,
    per row, a differently scaled, shifted and noised copy of it.  With the default texture the 4 x 4 blocks are nearly flat: sx + sy falls
    to the order of C2 and cs takes either sign there -- the ill-conditioned end, right for bit-exact comparisons."""
    rng = np.random.RandomState(seed)
    b, c, h, w = shape
    coarse = rng.uniform(-1, 1, (b, c, (h + 3) // 4, (w + 3) // 4))
    x = np.kron(coarse, np.ones((4, 4)))[..., :h, :w] * (1.0 - texture) + rng.uniform(-texture, texture, shape)
    ys = []
    for r in range(rows or 1):
        gain, bias, noise = 1.0 - 0.15 * r, 0.05 * r - 0.05, 0.05 + 0.1 * r
        ys.append(np.clip(gain * x + bias + rng.normal(0, noise, shape), -1, 1))
    y = np.stack(ys) if rows else ys[0]
    return x.astype(np.float32), y.astype(np.float32)


def pair_u8(shape, seed, rows=None):
    """The same as uint8 values (value_range "uint8")."""
    x, y = pair(shape, seed, rows)
    return np.round((x + 1) * 127.5).astype(np.uint8), np.round((y + 1) * 127.5).astype(np.uint8)


def single_scale_shapes(th, tw):
    """(H, W, k) around the kernel's th x tw output tile: one output pixel, the smallest window, one output column, a tile minus and plus a
    pixel on each axis, two tile rows plus a pixel."""
    k = 11
    return [(11, 11, 11), (3, 4, 3), (40, 11, 11), (th + k - 2, tw + k, k), (th + k, tw + k - 2, k), (2 * th + k, tw + k - 1, k)]


# (H, W, k): odd padding on every level and a last map of 1 x 1 (33 -> 17 -> 9 -> 5 -> 3 with k = 3; 161 -> 81 -> 41 -> 21 -> 11 with k = 11)
MS_SHAPES = [(33, 35, 3), (34, 33, 3), (161, 161, 11)]

POOLED = {224: [224, 112, 56, 28, 14], 161: [161, 81, 41, 21, 11], 33: [33, 17, 9, 5, 3], 35: [35, 18, 9, 5, 3]}
