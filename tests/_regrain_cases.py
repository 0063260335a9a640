"""Inputs shared by tests/test_regrain_cpu.py and tests/test_gpu_regrain.py, all drawn from fixed seeds."""
import numpy as np

# (h, w, n_iters, min_side) -> the sizes of the levels
LEVEL_CASES = [
    ((224, 224, 6, 20), [(224, 224), (112, 112), (56, 56), (28, 28)]),
    ((42, 42, 6, 20), [(42, 42), (21, 21)]),
    ((40, 40, 6, 20), [(40, 40)]),
    ((9, 7, 3, 0), [(9, 7), (5, 4), (3, 2)]),
    ((1, 1, 3, 0), [(1, 1), (1, 1), (1, 1)]),
    ((512, 512, 6, 20), [(512, 512), (256, 256), (128, 128), (64, 64), (32, 32)]),
    ((224, 30, 6, 20), [(224, 30)]),
]

# (h, w, iters, min_side, smoothness) of the kernel-level comparisons.  The solve keeps regions of at most 4096 cells (64 x 64 when tiled)
# and runs at most 8 iterations per tiled launch on owned tiles of 48 x 48: (150, 170) with 9 iterations is three tiles and a remainder both
# ways at the deepest halo, then a launch of one iteration on 62 x 62 tiles; its second level, 75 x 85, is tiled as well.
ABI_CASES = [
    (1, 1, (3,), 20, 1.0),
    (1, 7, (3,), 20, 1.0),
    (2, 3, (2,), 20, 1.0),
    (7, 1, (5,), 20, 1.0),
    (9, 7, (2, 3, 4), 0, 1.0),
    (33, 18, (2, 3, 4), 0, 1.0),
    (150, 170, (9, 3), 0, 1.0),
    (70, 150, (5, 3), 0, 4.0),
    (42, 42, (4, 16, 32, 64, 64, 64), 20, 1.0),
    (48, 40, (4, 16), 20, 0.25),
]


def pair(b, h, w, seed, spread=0.25):
    """(original, transferred), both (b, 3, h, w) float64 in [0, 1] units: a smooth scene under texture, and a recoloured copy of it with
    banding and fresh noise, reaching ``spread`` beyond [0, 1]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx / max(w - 1, 1), yy / max(h - 1, 1), 0.5 + 0.4 * np.sin(xx / 5.0 + yy / 9.0)])
    i0 = np.clip(base[None] + 0.03 * rng.randn(b, 3, h, w), 0.0, 1.0)
    it = np.round(8 * i0[:, ::-1] ** 1.5) / 8 * (1 + 2 * spread) - spread + 0.02 * rng.randn(b, 3, h, w)
    return np.ascontiguousarray(i0), np.ascontiguousarray(it)


def grain_fixture(seed=7, h=96, w=120):
    """(I0, clean, IT), each (3, h, w): ramps and a sine with a brighter box under 0.02 randn texture; ``clean`` a mild monotone map of I0 per
    channel; IT = clean quantised to 12 steps plus 0.02 randn -- the banding and grain an iterated transfer leaves in flat regions."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    i0 = np.stack([0.15 + 0.7 * xx / (w - 1), 0.15 + 0.7 * yy / (h - 1), 0.5 + 0.3 * np.sin(xx / 11.0) * np.cos(yy / 13.0)])
    i0[:, 30:60, 40:90] += 0.12
    i0 = i0 + 0.02 * rng.randn(3, h, w)
    clean = np.stack([i0[0] ** 0.8, 0.1 + 0.8 * i0[1], np.sqrt(np.maximum(i0[2], 0.0))])
    it = np.round(12 * clean) / 12 + 0.02 * rng.randn(3, h, w)
    return i0, clean, it


def point_set(n, seed, cond=1e-4):
    """(3, n) float64 whose covariance has every eigenvalue at or above ``cond`` of the largest (about sqrt(cond) per axis)."""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.randn(3, 3))
    scale = np.array([0.2, 0.2 * cond ** 0.25 * 1.5, 0.2 * cond ** 0.5 * 1.5])
    return rng.uniform(0.3, 0.7, (3, 1)) + q @ (scale[:, None] * rng.randn(3, n))
