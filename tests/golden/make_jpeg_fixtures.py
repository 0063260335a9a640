"""Writes tests/golden/jpeg/: the JPEG / PNG files the JPEG tests need but the Pillow on a test machine may not be able to write
(restart intervals are recent Pillow options), each with the RGB array Pillow decoded from it where this script ran (expected.npz).
Everything comes from seeded arrays; nothing is read from elsewhere.

    python tests/golden/make_jpeg_fixtures.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _jpeg_ref import synth  # noqa: E402

OUT = os.path.join(HERE, "jpeg")


def main():
    os.makedirs(OUT, exist_ok=True)
    img = synth(52, 70, 7)
    files = {}

    def jpeg(name, im, **kw):
        f = io.BytesIO()
        im.save(f, "JPEG", **kw)
        files[name] = f.getvalue()

    rgb = Image.fromarray(img)
    jpeg("restart_blocks.jpg", rgb, quality=80, restart_marker_blocks=2)
    jpeg("restart_rows.jpg", rgb, quality=80, subsampling=1, restart_marker_rows=1)
    jpeg("restart_grey.jpg", Image.fromarray(img[..., 0]), quality=70, restart_marker_blocks=1)
    jpeg("progressive.jpg", rgb, quality=80, progressive=True)
    jpeg("cmyk.jpg", rgb.convert("CMYK"), quality=80)
    # 4:4:0 (luma 1x2): Pillow does not write it.  A 32 x 32 4:2:2 file has as many MCUs (2 x 4) as a 32 x 32 4:4:0 file (4 x 2), each
    # with the same blocks, so changing the luma sampling byte of its SOF0 from 0x21 to 0x12 gives a VALID 4:4:0 file (of another picture)
    jpeg("s440.jpg", Image.fromarray(synth(32, 32, 9)), quality=80, subsampling=1)
    at = files["s440.jpg"].index(b"\xff\xc0")
    assert files["s440.jpg"][at + 11] == 0x21
    files["s440.jpg"] = files["s440.jpg"][:at + 11] + b"\x12" + files["s440.jpg"][at + 12:]
    jpeg("baseline_420.jpg", rgb, quality=80)
    files["truncated.jpg"] = files["baseline_420.jpg"][:len(files["baseline_420.jpg"]) * 3 // 5]
    f = io.BytesIO()
    rgb.save(f, "PNG")
    files["rgb.png"] = f.getvalue()
    f = io.BytesIO()
    Image.fromarray(img[..., 1]).save(f, "PNG")
    files["grey.png"] = f.getvalue()

    expected = {}
    for name, data in files.items():
        with open(os.path.join(OUT, name), "wb") as fh:
            fh.write(data)
        if name != "truncated.jpg":
            expected[name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        print(f"{name}: {len(data)} bytes")
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)


if __name__ == "__main__":
    main()
