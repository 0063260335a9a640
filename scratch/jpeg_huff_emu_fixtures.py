"""Files for scratch/jpeg_huff_emu.cpp:  python scratch/jpeg_huff_emu_fixtures.py OUTDIR

The grid of tests/_jpeg_ref.py over the sizes of the device Huffman tests and every variant, the JPEG fixtures of tests/golden/jpeg
(restart intervals, the truncated file, the ones the parser refuses) and the black/white noise image that is over the magnitude bound.
The emulation needs no expected output: the host decoder compiled into it is the reference."""
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_ref as R  # noqa: E402

SIZES = [(1, 1), (8, 8), (16, 16), (33, 17), (97, 131), (64, 48), (7, 5), (3, 40), (40, 3)]


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, data in R.grid(SIZES):
        with open(os.path.join(out, f"grid_{name}.jpg"), "wb") as fh:
            fh.write(data)
    gold = os.path.join(ROOT, "tests", "golden", "jpeg")
    for f in sorted(os.listdir(gold)):
        if f.endswith(".jpg"):
            shutil.copy(os.path.join(gold, f), os.path.join(out, f"golden_{f}"))
    noise = (np.random.default_rng(7).integers(0, 2, (64, 64, 1)) * 255).astype(np.uint8).repeat(3, 2)
    with open(os.path.join(out, "noise_64x64_q100.jpg"), "wb") as fh:
        fh.write(R.encode(noise, dict(quality=100, subsampling=0)))


if __name__ == "__main__":
    main(sys.argv[1])
