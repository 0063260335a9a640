"""The images of the LZ77 tests (tests/test_png_lz_cpu.py, tests/test_gpu_png_lz.py): the smallest shapes at which each mechanism of
the matcher, the parse and the two-alphabet block can go wrong.  The restatement is pure Python per byte, so nothing is larger than
200 x 300.  ``computed(name)`` runs the restatement once per case and process; both test files share it."""
import numpy as np

import _png_enc_ref as R
import _png_lz_ref as L


def _copied_rows():
    """102 x 100 noise, rows 100-101 copied from rows 0-1: filtered row 101 equals filtered row 1 (same pixels, same prior row), at the
    distance 100 * 301 = 30100 inside the one segment -- distance code 29, 13 extra bits; 301 bytes do not fit one match."""
    img = R.make_image(102, 100, "noise")
    img[100:102] = img[0:2]
    return img


def _cell_grid():
    """3 x 3 cells of 24 x 24 gradient_noise, 2 px black padding all round, the third column a copy of the first (a demo table's input
    column): mid-range distances, literals and matches mixed, both codes with many symbols."""
    cell, pad, rows, cols = 24, 2, 3, 3
    out = np.zeros((rows * (cell + pad) + pad, cols * (cell + pad) + pad, 3), np.uint8)
    for r in range(rows):
        for c in range(cols):
            src = R.make_image(cell, cell, "gradient_noise", seed=10 * r + (c % 2))
            y, x = pad + r * (cell + pad), pad + c * (cell + pad)
            out[y:y + cell, x:x + cell] = src
    return out


def _clipped_ramp():
    """40 x 64 ramp, the top 12 rows clipped to 255: row-stride candidates across the filter-type bytes."""
    img = R.make_image(40, 64, "gradient")
    img[:12] = 255
    return img


CASES = {
    "1x1_noise": lambda: R.make_image(1, 1, "noise"),
    "99x110_gradient_noise": lambda: R.make_image(99, 110, "gradient_noise"),
    "64x64_noise": lambda: R.make_image(64, 64, "noise"),
    "16x16_flat": lambda: R.make_image(16, 16, "flat"),
    "1x300_flat": lambda: R.make_image(1, 300, "flat"),
    "128x85_flat": lambda: R.make_image(128, 85, "flat"),
    "128x86_flat": lambda: R.make_image(128, 86, "flat"),
    "102x100_noise_rows_copied": _copied_rows,
    "grid_3x3_of_24": _cell_grid,
    "40x64_ramp_clipped": _clipped_ramp,
    "8x8_saturated": lambda: R.make_image(8, 8, "saturated"),
    "200x300_natural": lambda: R.make_image(200, 300, "natural"),
}
NAMES = list(CASES)
NO_MATCH = ("1x1_noise", "99x110_gradient_noise", "64x64_noise")       # no match is chosen: the file is _png_enc_ref.encode's

_cache = {}


def computed(name):
    """(image, stages of the LZ77 restatement, the literal-only file), computed once."""
    if name not in _cache:
        img = CASES[name]()
        _cache[name] = (img, L.stages(img), R.encode(img))
    return _cache[name]


def dump(directory):
    """Writes NAME.in (int32 h, w, the filtered stream) and NAME.want (per segment int32 mode, int32 n, the n bytes) for
    scratch/png_lz_emu.cpp; returns the number of cases."""
    import os
    import struct
    os.makedirs(directory, exist_ok=True)
    for name in NAMES:
        img, st, _ = computed(name)
        with open(os.path.join(directory, name + ".in"), "wb") as fh:
            fh.write(struct.pack("<ii", img.shape[0], img.shape[1]) + st["filtered"])
        with open(os.path.join(directory, name + ".want"), "wb") as fh:
            for seg, mode in zip(st["segments"], st["modes"]):
                fh.write(struct.pack("<ii", mode, len(seg)) + seg)
    return len(NAMES)
