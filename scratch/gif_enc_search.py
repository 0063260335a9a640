"""Finds the sizes of tests/_gif_enc_cases.py's PAYLOAD_255: trims of the natural tile whose LZW payload is 0 and 1 (mod 255) bytes long.
    python scratch/gif_enc_search.py
Also decodes every case's restatement file with Pillow, as a first check after a change of the format."""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _gif_enc_cases as C  # noqa: E402
import _gif_enc_ref as R  # noqa: E402


def main():
    from PIL import Image, ImageSequence
    for name in C.CASES:
        data, info = C.expected(name)
        im = Image.open(io.BytesIO(data))
        got = [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)]
        order = C.CASES[name].order or range(len(info))
        ok = len(got) == len(order) and all(np.array_equal(g, info[i]["palette"][info[i]["index"]]) for g, i in zip(got, order))
        print(f"{name}: {len(data)} bytes, {len(got)} frames, decodes to palette[index]: {ok}")
    found = {}
    tile = C.natural(40, 60)
    for h in range(40, 8, -1):
        for w in range(60, 20, -1):
            k = R.image_block(tile[:h, :w], 10)[1]["payload"]
            if k > 255 and k % 255 in (0, 1) and k % 255 not in found:
                found[k % 255] = (h, w)
                print(f"payload {k} = 255 * {k // 255} + {k % 255} at {h} x {w}")
        if len(found) == 2:
            break
    print("PAYLOAD_255 =", found)


if __name__ == "__main__":
    main()
