"""Inputs and the case list shared by tests/test_guided_cpu.py and tests/test_gpu_guided.py: seeded and TEXTURED (a flat guide makes Sigma
equal eps 1 and hides indexing errors), the smallest shapes at which csrc/guided.hip can still go wrong."""
import numpy as np


def guide(n, hl, wl, seed, texture=0.25):
    """(N, 3, hl, wl) float32 in [-1, 1]: per channel a blocky random picture under uniform noise."""
    rng = np.random.RandomState(seed)
    coarse = rng.uniform(-1, 1, (n, 3, (hl + 3) // 4, (wl + 3) // 4))
    x = np.kron(coarse, np.ones((4, 4)))[..., :hl, :wl] * (1.0 - texture) + rng.uniform(-texture, texture, (n, 3, hl, wl))
    return x.astype(np.float32)


def targets(g, rows, seed):
    """(R, N, 3, hl, wl) float32 in [0, 1]: per row a different colour mix of the guide plus a smooth ramp and noise -- what a network that
    changes the appearance and keeps the scene returns."""
    rng = np.random.RandomState(seed + 1000)
    n, _, hl, wl = g.shape
    g01 = g.astype(np.float64) * 0.5 + 0.5
    ramp = np.linspace(0.0, 1.0, hl)[:, None] * np.linspace(1.0, 0.0, wl)[None, :] if hl * wl > 1 else np.zeros((hl, wl))
    out = []
    for r in range(rows):
        mix = rng.uniform(-0.3, 0.9, (3, 3))
        t = np.einsum("ck,nkhw->nchw", mix, g01) * 0.6 + 0.2 * ramp + rng.normal(0, 0.03 + 0.02 * r, g.shape) + 0.05 * r
        out.append(np.clip(t, 0, 1))
    return np.stack(out).astype(np.float32)


def photo_batch(sizes, seed):
    """Padded (N, Hmax, Wmax, 3) uint8 batch of textured photographs of the given (h, w); the padding holds 0x5A."""
    rng = np.random.RandomState(seed + 2000)
    hmax, wmax = max(h for h, _ in sizes), max(w for _, w in sizes)
    out = np.full((len(sizes), hmax, wmax, 3), 0x5A, dtype=np.uint8)
    for i, (h, w) in enumerate(sizes):
        coarse = rng.uniform(0, 255, ((h + 5) // 6, (w + 5) // 6, 3))
        img = np.kron(coarse, np.ones((6, 6, 1)))[:h, :w] * 0.7 + rng.uniform(0, 76, (h, w, 3))
        out[i, :h, :w] = np.clip(img, 0, 255).astype(np.uint8)
    return out


# target layouts (tfmt): "nchw" fp32, "nhwc" fp32 channels-last (the sweep's output), "bf16", "slice" (a strided slice of a larger tensor);
# guide layouts (gfmt): "contig", or "strided" (a channels-last crop of a larger tensor)


def coefficient_cases(th, tw):
    """dict(hl, wl, r, eps, n, rows, tfmt, gfmt) around the th x tw tile of wu_guided_tile_h / _w: the degenerate 1 x 1 and 1 x 9 images,
    small odd sizes, hl x wl one below, at and one above the tile, r in {0, 1, 3} and r >= max(hl, wl), eps in {1e-6, 1e-3, 1e-2},
    R in {1, 3}, every target and guide layout."""
    rows = [
        (1, 1, 0, 1e-3, 1, 1, "nchw", "contig"),
        (1, 1, 3, 1e-6, 2, 3, "nhwc", "contig"),                 # r >= max(hl, wl) on a single pixel
        (1, 9, 1, 1e-2, 1, 3, "nhwc", "strided"),
        (7, 5, 3, 1e-6, 2, 3, "bf16", "contig"),
        (7, 5, 9, 1e-3, 1, 1, "nchw", "contig"),                 # r >= max(hl, wl): one global regression
        (32, 40, 3, 1e-3, 2, 3, "slice", "strided"),
        (32, 40, 1, 1e-6, 1, 1, "nchw", "contig"),
        (32, 40, 40, 1e-2, 1, 1, "bf16", "contig"),              # r = max(hl, wl)
        (40, 33, 8, 1e-3, 1, 3, "nchw", "contig"),               # the largest radius of the tiled smoothing pass, 2 x 2 of its tiles
        (40, 33, 9, 1e-3, 2, 1, "nhwc", "contig"),               # one above it: the two-pass form
        (th - 1, tw - 1, 1, 1e-2, 1, 1, "nchw", "contig"),
        (th, tw, 0, 1e-3, 1, 3, "nhwc", "contig"),
        (th + 1, tw + 1, 3, 1e-6, 2, 1, "slice", "contig"),
    ]
    keys = ("hl", "wl", "r", "eps", "n", "rows", "tfmt", "gfmt")
    return [dict(zip(keys, row)) for row in rows]


def apply_cases(th, tw):
    """dict(hl, wl, sizes, rows): photographs of 1 x 1, 3 x 200, 97 x 131 (alone under one row, in a batch under three), h == hl, h < hl
    (mildly: the patch stays on chip; strongly: it does not), sizes one below, at and one above the apply tile as a padded batch of three
    different sizes, R in {1, 3}, low-resolution 1 x 1 and 1 x 9 maps.  Both kernel variants of the launcher (largest tile patch below and
    from 32 entries) meet one row and three rows."""
    rows = [
        (7, 5, [(1, 1)], 1),
        (7, 5, [(3, 200)], 3),
        (32, 40, [(97, 131)], 1),
        (32, 40, [(97, 131), (50, 31)], 3),                      # patches of 84 entries and more: requested a row ahead, three rows
        (32, 40, [(32, 40)], 3),                                 # h == hl: the plain guided filter, tap weights 0
        (32, 40, [(20, 30)], 1),                                 # h < hl, patch within the on-chip budget
        (32, 40, [(9, 11), (32, 40)], 3),                        # h << hl next to h == hl: the patch of a tile exceeds the budget
        (32, 40, [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1)], 3),
        (32, 40, [(2 * th + 1, tw + 1), (th, 2 * tw + 1), (5, 7)], 1),
        (1, 1, [(5, 7)], 1),
        (1, 9, [(4, 70)], 3),
    ]
    return [dict(zip(("hl", "wl", "sizes", "rows"), row)) for row in rows]


def case_inputs(case, seed):
    """(guide (N, 3, hl, wl), targets (R, N, 3, hl, wl)) float32 of a case."""
    n = case.get("n", len(case.get("sizes", [0])))
    g = guide(n, case["hl"], case["wl"], seed)
    return g, targets(g, case["rows"], seed)
