"""Inputs and shapes shared by tests/test_swd_cpu.py and tests/test_gpu_swd.py."""
import numpy as np

# (H, W, levels): one level (L = G, no up-sampling), two levels square and rectangular, three levels
GATHER_SHAPES = [(16, 16, 1), (32, 32, 2), (32, 48, 2), (64, 64, 3)]
GATHER_NP = [(1, 1), (1, 5), (3, 1), (3, 5)]

SORT_KINDS = ("random", "ascending", "descending", "equal", "duplicates")


def images(n, h, w, seed):
    """(n, 3, h, w) float32 in [-1, 1]: a blocky picture under noise, so that every pyramid level carries signal."""
    rng = np.random.RandomState(seed)
    coarse = rng.uniform(-1, 1, (n, 3, (h + 7) // 8, (w + 7) // 8))
    x = 0.6 * np.kron(coarse, np.ones((8, 8)))[..., :h, :w] + rng.uniform(-0.4, 0.4, (n, 3, h, w))
    return x.astype(np.float32)


def images_u8(n, h, w, seed):
    return np.round((images(n, h, w, seed) + 1) * 127.5).astype(np.uint8)


def level_shapes(h, w, levels):
    return [(h >> l, w >> l) for l in range(levels)]


def positions(n, p, h, w, levels, seed):
    """int32 (levels, n, p, 2): per level the four corner-most centres first -- (3, 3), (3, W_l - 4), (H_l - 4, 3), (H_l - 4, W_l - 4), so
    that the mirrored border of both passes is read -- spread over the (n, p) slots in order, then random centres inside the bounds."""
    rng = np.random.RandomState(seed)
    pos = np.empty((levels, n, p, 2), dtype=np.int32)
    for l, (hl, wl) in enumerate(level_shapes(h, w, levels)):
        flat = np.stack([rng.randint(3, hl - 3, size=n * p), rng.randint(3, wl - 3, size=n * p)], axis=1)
        corners = [(3, 3), (3, wl - 4), (hl - 4, 3), (hl - 4, wl - 4)]
        for k in range(min(4, n * p)):           # fewer than four slots: the two opposite corners first, rotated from level to level
            flat[k] = corners[(0, 3, 1, 2)[(k + l) % 4]]
        pos[l] = flat.reshape(n, p, 2)
    return pos


def sort_sizes(block):
    """m around the on-chip block b: the smallest sets, a wave, a block minus / plus a key, runs that need two and three merge passes with
    a ragged last run."""
    return [1, 2, 63, 64, 65, block - 1, block, block + 1, 2 * block + 17, 5 * block + 3]


def sort_columns(m, ncols, kind, seed):
    """(m, ncols) small integers as float32 (exact in any arithmetic), negative values included."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        v = rng.randint(-30000, 30000, size=(m, ncols))
    elif kind == "ascending":
        v = np.arange(m)[:, None] - m // 2 + np.arange(ncols)[None, :]
    elif kind == "descending":
        v = m // 3 - np.arange(m)[:, None] - np.arange(ncols)[None, :]
    elif kind == "equal":
        v = np.full((m, ncols), -7) + np.arange(ncols)[None, :]
    elif kind == "duplicates":
        v = rng.randint(-2, 3, size=(m, ncols))
    else:
        raise ValueError(kind)
    return v.astype(np.float32)


def one_hot_case(m, ncols, kind, seed):
    """(desc (m, 147) float32, dirs (ncols, 147) one-hot float32, columns (m, ncols)): every projection is exactly one descriptor column.
    The chosen feature indices are spread over 0..146, the last one included; the other features hold integer noise."""
    rng = np.random.RandomState(seed + 1)
    desc = rng.randint(-9, 10, size=(m, 147)).astype(np.float32)
    feats = np.array(([146, 0] + [int(f) for f in rng.permutation(147) if f not in (0, 146)])[:ncols])
    cols = sort_columns(m, ncols, kind, seed)
    desc[:, feats] = cols
    dirs = np.zeros((ncols, 147), dtype=np.float32)
    dirs[np.arange(ncols), feats] = 1.0
    return desc, dirs, cols


def normalised_descriptors(m, seed):
    """(m, 147) float32, roughly unit variance per entry, like normalised Laplacian patches."""
    return np.random.RandomState(seed).randn(m, 147).astype(np.float32)


def unit_dirs(ndirs, seed):
    d = np.random.RandomState(seed).randn(147, ndirs)
    d = d / np.sqrt(np.sum(np.square(d), axis=0, keepdims=True))
    return np.ascontiguousarray(d.astype(np.float32).T)
