"""Writes the fixtures of tests/_png_dec_cases.py for scratch/png_dec_emu.cpp:  python scratch/png_dec_emu_fixtures.py OUTDIR
NAME.png and NAME.want (int32 status; for status 0 then int32 h, int32 w and the pixels) -- status and pixels from the restatement
tests/_png_dec_ref.py, the pixels checked against Pillow."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _png_dec_cases as C  # noqa: E402
import _png_dec_ref as D  # noqa: E402


def main(out):
    os.makedirs(out, exist_ok=True)
    codes = {v: k for k, v in D.STATUS.items()}
    for name, case in C.CASES.items():
        verdict, px = C.expected(name)
        assert verdict in codes, (name, verdict)               # every fixture passes the parser
        assert verdict == (case.want or "ok"), (name, verdict)
        with open(os.path.join(out, name + ".png"), "wb") as fh:
            fh.write(case.file)
        with open(os.path.join(out, name + ".want"), "wb") as fh:
            fh.write(struct.pack("<i", codes[verdict]))
            if px is not None:
                assert np.array_equal(px, C.pillow(case.file)), name
                fh.write(struct.pack("<ii", px.shape[0], px.shape[1]) + px.tobytes())
    print(f"{len(C.CASES)} fixtures in {out}")


if __name__ == "__main__":
    main(sys.argv[1])
