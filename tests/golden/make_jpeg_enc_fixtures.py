"""Writes tests/golden/jpeg_enc/: a dozen tiny inputs (.npy, (h, w, 3) uint8) and the file Pillow wrote for each (.jpg).  They pin
the encoder's bytes against the Pillow / libjpeg of the machine that ran this script, so that a different Pillow elsewhere shows as
a fixture mismatch rather than as an encoder fault.  Names: {h}x{w}_{content}_q{quality}_{444|420}.  Run from the repository root:

    python tests/golden/make_jpeg_enc_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _jpeg_enc_ref as R          # noqa: E402

CASES = [(1, 1, "noise", 75, "4:2:0"), (7, 5, "gradient", 75, "4:2:0"), (8, 8, "saturated", 100, "4:2:0"), (12, 12, "noise", 30, "4:2:0"),
         (16, 16, "flat", 75, "4:2:0"), (17, 17, "noise", 100, "4:2:0"), (24, 40, "gradient", 30, "4:2:0"), (40, 24, "saturated", 75, "4:2:0"),
         (33, 1, "noise", 75, "4:2:0"), (3, 40, "gradient", 100, "4:4:4"), (50, 16, "noise", 75, "4:4:4"), (100, 75, "gradient", 75, "4:2:0")]


def name(h, w, content, quality, subsampling):
    return f"{h}x{w}_{content}_q{quality}_{subsampling.replace(':', '')}"


def main():
    out = os.path.join(HERE, "jpeg_enc")
    os.makedirs(out, exist_ok=True)
    total = 0
    for h, w, content, quality, subsampling in CASES:
        img = R.make_image(h, w, content)
        data = R.pillow_jpeg(img, quality, 0 if subsampling == "4:4:4" else 2)
        stem = os.path.join(out, name(h, w, content, quality, subsampling))
        np.save(stem + ".npy", img)
        with open(stem + ".jpg", "wb") as fh:
            fh.write(data)
        total += os.path.getsize(stem + ".npy") + len(data)
    print(f"{len(CASES)} fixtures, {total} bytes")


if __name__ == "__main__":
    main()
