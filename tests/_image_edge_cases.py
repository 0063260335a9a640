"""The cases of tests/test_input_edges_cpu.py and tests/test_gpu_input_edges.py: batches for wu.input_pipeline.GPUInputPipeline with EXPLICIT
per-image parameters (the dicts ``draw()`` returns), at the edges random draws of the default ranges never reach.  One list, so the numpy
restatement (tests/_image_ref.py, on any machine) and the HIP kernels (on the GPU) are held to Pillow on the very same inputs.  CPU work
only; imports nothing of the HIP library.

A case is one batch: sizes, S, params, augmentation, train, and the (Hmax, Wmax) of the padded buffer.  Sources come from a seeded
generator; the PADDING of the buffer is never zero (zero looks like Image.rotate's black fill and like a clipped tap): ``padded(case,
"255")`` and ``padded(case, "noise")`` give the two poisoned buffers.  Every S <= 64.

    geo_*      resize only (train=False, and augmentation=False with angle 0): 1-pixel sources, identity, exact 2x / 3x, a 128.9x
               down-scale sharing its ksize with up-scaling images, S = 1, S = 33 (N*S*S no multiple of the 256-thread block)
    crop_*     RandomResizedCrop windows on a 45 x 70 image in a 64 x 96 buffer: 1 x 1 corners, last row / column, full, flush bottom-right
    rot_*      angles -10, 10, 0, +-360, 1e-7, 90, 180, 270, 45: after the resize (S x S) and before it (37 x 53 source, corner crop)
    jit_*      the enhancers at S*S below / no multiple of / a multiple of the 1024-thread block: a factor grid that holds the values at
               which a fused blend and Pillow's two-step blend disagree, all orders and partial orders, flat / saturated / tie-mean images
"""
from collections import namedtuple

import numpy as np

from oracle import input_ref as IR

Case = namedtuple("Case", "name S sizes params augmentation train buf_hw images tags")
CASES = {}

NO_JITTER = {"factors": (1.0, 1.0, 1.0), "order": (-1, -1, -1)}
IDENTITY_JITTER = {"factors": (1.0, 1.0, 1.0), "order": (0, 1, 2)}
GRID = (0.0, 0.5, 2.0 / 3.0, 0.8, 1.0, 1.1, 1.2, 4.0 / 3.0, 1.5, 2.0)
SENSITIVE = (0.8, 1.1, 1.2, 2.0 / 3.0, 4.0 / 3.0)       # float32(f) sits just above a short rational: one rounding != two roundings
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0), (1, -1, -1), (-1, 2, -1), (2, 1, -1))
ANGLES = (-10.0, 10.0, 0.0, 360.0, -360.0, 1e-7, 90.0, 180.0, 270.0, 45.0)
NO_ROTATION = (0.0, 360.0, -360.0)                       # Image.rotate returns a copy: the product must not rotate either


def textured(h, w, i, rng):
    """The smooth + noise image of tests/test_gpu_input.py's _batch."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + i), 128 + 90 * np.cos(yy / 5.0), 40 + (xx + yy) % 200], -1)
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _flat(h, w, rgb):
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


def _half(h, w, k, n_hi):
    """Grey k with n_hi pixels of grey k + 1, scattered: mean grey = k + n_hi / (h * w)."""
    g = np.full(h * w, k, np.uint8)
    g[np.random.default_rng(h * w).permutation(h * w)[:n_hi]] = k + 1
    return np.repeat(g.reshape(h, w, 1), 3, 2)


def special(kind, h, w, rng):
    n = h * w
    if kind == "textured":
        return textured(h, w, 0, rng)
    if kind == "ramp":
        return np.repeat((np.arange(n) * 255 // max(n - 1, 1)).astype(np.uint8).reshape(h, w, 1), 3, 2)
    if kind == "half":                                   # even n: the mean is exactly 100.5; odd n: just below it
        return _half(h, w, 100, n // 2)
    if kind == "half_up":                                # odd n: just above 100.5
        return _half(h, w, 100, (n + 1) // 2)
    if kind == "dark":                                   # mean grey near 12: Contrast's degenerate sits beside the clip at 0
        return np.clip(12 + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
    if kind == "bright":                                 # mean grey near 240
        return np.clip(240 + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)
    return _flat(h, w, {"black": (0, 0, 0), "white": (255, 255, 255), "red": (255, 0, 0), "green": (0, 255, 0), "blue": (0, 0, 255)}[kind])


def _add(name, S, sizes, params, augmentation, train, buf_hw=None, images=None, tags=None):
    assert name not in CASES and S <= 64 and len(sizes) == len(params)
    rng = np.random.default_rng(7000 + len(CASES))
    if images is None:
        images = [textured(h, w, i, rng) for i, (h, w) in enumerate(sizes)]
    hmax, wmax = max(h for h, _ in sizes), max(w for _, w in sizes)
    buf_hw = buf_hw or (hmax, wmax)
    assert buf_hw[0] >= hmax and buf_hw[1] >= wmax
    assert all(im.shape == (h, w, 3) and im.dtype == np.uint8 for im, (h, w) in zip(images, sizes))
    params = [{"angle": 0.0, "flip": False, "crop": (0, 0, h, w), **NO_JITTER, **p} for p, (h, w) in zip(params, sizes)]
    CASES[name] = Case(name, S, [tuple(s) for s in sizes], params, augmentation, train, buf_hw, images, tags or [None] * len(sizes))
    return CASES[name]


def padded(case, fill):
    """The (N, Hmax, Wmax, 3) uint8 buffer with the sources top-left and poison elsewhere: fill = "255" or "noise"."""
    shape = (len(case.sizes), *case.buf_hw, 3)
    if fill == "255":
        buf = np.full(shape, 255, np.uint8)
    else:
        assert fill == "noise"
        buf = np.random.default_rng(len(case.name)).integers(1, 256, shape, dtype=np.uint8)
    for i, ((h, w), im) in enumerate(zip(case.sizes, case.images)):
        buf[i, :h, :w] = im
    return buf


_pillow = {}


def pillow(name):
    """(N, 3, S, S) float32: the Pillow chain on every image of the case, computed once.  Treat as read-only."""
    if name not in _pillow:
        c = CASES[name]
        out = []
        for im, p in zip(c.images, c.params):
            if c.train:
                out.append(IR.train_transform(im, c.S, p["angle"], p["flip"], c.augmentation, p["crop"], p["factors"], p["order"]))
            else:
                out.append(IR.test_transform(im, c.S))
        _pillow[name] = np.stack(out)
        _pillow[name].setflags(write=False)
    return _pillow[name]


def first_difference(case, got, want):
    """'' if equal; else, per differing image, its parameters, the count and largest size of the differences (in bytes: 2 / 255 of
    the normalised range each) and the first differing (n, c, y, x)."""
    if got.shape != want.shape:
        return f"{case.name}: shape {got.shape} != {want.shape}"
    bad = (got != want) | np.isnan(got)
    lines = []
    for n in np.flatnonzero(bad.reshape(len(bad), -1).any(1)):
        c, y, x = (int(v) for v in np.argwhere(bad[n])[0])
        lines.append(f"{case.name}[{n}] size {case.sizes[n]} S {case.S} aug {case.augmentation} train {case.train} {case.params[n]}: "
                     f"{int(bad[n].sum())} of {bad[n].size} values differ, largest by {np.nanmax(np.abs(got[n] - want[n])) * 127.5:.2f} bytes; "
                     f"first at (n, c, y, x) = ({n}, {c}, {y}, {x}): got {got[n, c, y, x]!r}, want {want[n, c, y, x]!r}")
    return "\n".join(lines)


# =================================================================================================
# geometry without rotation
# =================================================================================================
MIXED = [(1, 1), (1, 37), (41, 1), (8, 8), (16, 24), (257, 1031)]          # at S = 8: up-scales, identity, exact 2x and 3x, 32.1x / 128.9x
UPSCALING = MIXED[:3]                                                      # the images whose own ksize is 3
for S in (8, 1):
    _add(f"geo_mixed_S{S}_test", S, MIXED, [{}] * 6, False, False)
    _add(f"geo_mixed_S{S}_train", S, MIXED, [{"flip": bool(i % 2)} for i in range(6)], False, True)
_add("geo_upscale_S8_test", 8, UPSCALING, [{}] * 3, False, False, buf_hw=(43, 39))
ODD = [(50, 33), (33, 66), (20, 100)]                                       # S = 33: 1.5x down / identity, identity / exact 2x, up / 3.03x
assert (len(ODD) * 33 * 33) % 256 != 0
_add("geo_S33_test", 33, ODD, [{}] * 3, False, False)
_add("geo_S33_train_unflipped", 33, ODD, [{"flip": False}] * 3, False, True)
_add("geo_S33_train_flipped", 33, ODD, [{"flip": True}] * 3, False, True)
GEOMETRY_CASES = [n for n in CASES]

# =================================================================================================
# crop windows: a 45 x 70 image inside a 64 x 96 buffer, S = 16, identity jitter (the u8 staging path)
# =================================================================================================
CROP_HW = (45, 70)
WINDOWS = [(0, 0, 1, 1), (0, 69, 1, 1), (44, 0, 1, 1), (44, 69, 1, 1), (44, 0, 1, 70), (0, 69, 45, 1), (0, 0, 45, 70), (42, 65, 3, 5)]
for flip in (False, True):
    _add(f"crop_windows_{'flipped' if flip else 'unflipped'}", 16, [CROP_HW] * len(WINDOWS),
         [{"crop": w, "flip": flip, **IDENTITY_JITTER} for w in WINDOWS], True, True, buf_hw=(64, 96))
CROP_CASES = [n for n in CASES if n.startswith("crop_")]

# =================================================================================================
# rotation
# =================================================================================================
for S in (16, 33):                                                          # Resize -> rotate the S x S image (90 / 180 / 270: PIL transposes)
    _add(f"rot_after_S{S}", S, [(37, 53)] * len(ANGLES), [{"angle": a, "flip": bool(i % 3 == 1)} for i, a in enumerate(ANGLES)], False, True,
         buf_hw=(40, 64))
# rotate the non-square source (90 / 270 stay affine maps: black bands left and right), then crop: the top-left corner window holds
# rotated-in black for every real rotation, the full window holds all four corners
_add("rot_before_corner", 16, [(37, 53)] * len(ANGLES), [{"angle": a, "crop": (0, 0, 20, 30), "flip": bool(i % 3 == 1)} for i, a in enumerate(ANGLES)],
     True, True, buf_hw=(40, 64))
_add("rot_before_full", 16, [(37, 53)] * len(ANGLES), [{"angle": a, "flip": bool(i % 3 == 2), **IDENTITY_JITTER} for i, a in enumerate(ANGLES)],
     True, True, buf_hw=(40, 64))
ROTATION_CASES = [n for n in CASES if n.startswith("rot_")]

# =================================================================================================
# colour jitter: S x S sources resized 1:1 (the staged image IS the source), in a buffer with a poisoned margin
# =================================================================================================
OP_ORDER = {0: (0, -1, -1), 1: (1, -1, -1), 2: (-1, 2, -1)}                 # one enhancer alone, through the partial orders
OP_NAME = {0: "Brightness", 1: "Contrast", 2: "Color"}
SPECIALS = ("black", "white", "red", "green", "blue", "ramp", "half", "dark", "bright")
SPECIAL_FACTORS = ((0.0, 0.0, 0.0), (2.0, 2.0, 2.0), (0.5, 1.5, 0.0), (1.0, 1.0, 1.0), (1.2, 0.8, 4.0 / 3.0), (1.5, 2.0 / 3.0, 1.1))
MIXES = ((0.8, 1.1, 1.2), (1.5, 2.0 / 3.0, 4.0 / 3.0), (0.5, 1.2, 0.8), (2.0, 0.0, 1.1), (1.1, 4.0 / 3.0, 0.0), (0.0, 1.5, 2.0),
         (4.0 / 3.0, 0.8, 2.0 / 3.0), (1.0, 1.1, 1.0), (2.0 / 3.0, 2.0, 0.5))


def _jitter_case(name, S, entries):
    """entries: (image kind, factors, order, tag)."""
    rng = np.random.default_rng(S * 1000 + len(CASES))
    images = [special(kind, S, S, rng) if kind != "textured" else textured(S, S, i, rng) for i, (kind, _, _, _) in enumerate(entries)]
    return _add(name, S, [(S, S)] * len(entries), [{"factors": tuple(f), "order": tuple(o)} for _, f, o, _ in entries], True, True,
                buf_hw=(S + 3, S + 5), images=images, tags=[t for _, _, _, t in entries])


for S in (8, 33, 64):
    assert (S * S < 1024, S * S % 1024 != 0) == {8: (True, True), 33: (False, True), 64: (False, False)}[S]
    # every factor of the grid alone under each enhancer on the textured image; tag = (enhancer, factor)
    single = []
    for op in (0, 1, 2):
        for f in GRID:
            fac = [1.0, 1.0, 1.0]
            fac[op] = f
            single.append(("textured", fac, OP_ORDER[op], (OP_NAME[op], f)))
    _jitter_case(f"jit_single_S{S}", S, single)
    # every order and partial order on the textured image, the sensitive factors mixed in
    _jitter_case(f"jit_orders_S{S}", S, [("textured", MIXES[i], o, None) for i, o in enumerate(ORDERS)])
    # flat, saturated, tie-mean, dark and bright images: the clip branch, factor 0 and 1, mean grey on k + 0.5
    kinds = SPECIALS + (("half_up",) if S % 2 else ())
    _jitter_case(f"jit_special_S{S}", S, [(kind, SPECIAL_FACTORS[(i + j) % len(SPECIAL_FACTORS)], ORDERS[(i * 3 + j) % len(ORDERS)], None)
                                          for i, kind in enumerate(kinds) for j in range(4)])
JITTER_CASES = [n for n in CASES if n.startswith("jit_")]
# where one image is big enough for a handful of one-byte differences to be certain (S = 8 has 192 bytes: too few to promise one)
PREMISE_CASES = ["jit_single_S33", "jit_single_S64"]

ALL_CASES = list(CASES)
assert sorted(ALL_CASES) == sorted(GEOMETRY_CASES + CROP_CASES + ROTATION_CASES + JITTER_CASES)
