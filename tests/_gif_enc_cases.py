"""The cases of the GIF encoder's tests (tests/test_gif_enc_cpu.py, tests/test_gpu_gif_enc.py; scratch/gif_enc_emu.cpp reads them through
``dump``), each with the restatement's file and stats computed once.  Every case is ASSERTED here to reach the edge it is named for: a case
that stops exercising its edge fails at import instead of passing for nothing."""
import os
import struct
from collections import namedtuple

import numpy as np

import _gif_enc_ref as R

GOLDEN_JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")

# base: the array the frames are a view of; view: the index that makes them (None: the whole base).  lossless: must decode to the input.
Case = namedtuple("Case", "base view duration_ms loop order lossless")
CASES = {}
_done = {}


def frames(name):
    c = CASES[name]
    return c.base if c.view is None else c.base[c.view]


def expected(name):
    """(file, per-frame info) of the restatement, computed once."""
    if name not in _done:
        c = CASES[name]
        _done[name] = R.encode(frames(name), c.duration_ms, c.loop, c.order, stats=True)
    return _done[name]


def _add(name, base, view=None, duration_ms=100, loop=0, order=None, lossless=False):
    base = np.ascontiguousarray(base, dtype=np.uint8)
    if base.ndim == 3:
        base = base[None]
    CASES[name] = Case(base, view, duration_ms, loop, order, lossless)
    return expected(name)[1]


def colours(index):
    """index -> (8 (i % 32), 8 (i // 32) + 3, 200): 256 colours, one per histogram bin, so the frame is reproduced exactly and the LZW's
    hit / miss structure is that of the index stream whatever numbers the boxes get."""
    i = np.asarray(index, np.int64)
    return np.stack([8 * (i % 32), 8 * (i // 32) + 3, np.full_like(i, 200)], -1).astype(np.uint8)


def natural(h, w, at=(0, 0)):
    """A tile of the decoded baseline fixture, mirrored so that any size fits."""
    from PIL import Image
    a = np.asarray(Image.open(os.path.join(GOLDEN_JPEG, "baseline_420.jpg")).convert("RGB"))
    a = np.concatenate([a, a[:, ::-1]], 1)
    a = np.concatenate([a, a[::-1]], 0)
    a = np.tile(a, (-(-(h + at[0]) // a.shape[0]), -(-(w + at[1]) // a.shape[1]), 1))
    return a[at[0]:at[0] + h, at[1]:at[1] + w].copy()


# ---- 1 x 1 -------------------------------------------------------------------------------------------------------------------------------
info = _add("one_pixel", np.array([[[[9, 250, 77]]]]), lossless=False)
assert info[0]["boxes"] == 1 and len(info[0]["segments"]) == 1

# ---- 255 distinct colours: 254 misses, next == 512 at the end, so the end-of-information code goes out at 10 bits --------------------------
info = _add("colours_255", colours(np.arange(255).reshape(15, 17)), lossless=True)
seg = info[0]["segments"][-1]
assert info[0]["boxes"] == 255 and seg["next"] == 512 and seg["bump"] and seg["width"] == 10, seg

# ---- the width edges at a segment boundary: segment 0 ends at next == 512 / 1024 / 2048 exactly, the Clear behind it one bit wider ---------
EDGE_A = {128: 512, 645: 1024, 1690: 2048, 1000: None}               # a -> next at the end of segment 0 (None: the control, no bump)
for a, want in EDGE_A.items():
    idx = np.full(72 * 128, 255, np.int64)
    idx[:a] = np.random.default_rng(0).integers(0, 255, R.SEGMENT)[:a]
    idx[R.SEGMENT:] = np.random.default_rng(1).integers(0, 256, 1024)
    info = _add(f"width_edge_a{a}", colours(idx.reshape(72, 128)), lossless=True)
    seg = info[0]["segments"]
    assert len(seg) == 2
    if want is None:
        assert not seg[0]["bump"] and seg[0]["next"] not in (512, 1024, 2048), seg[0]
    else:
        assert seg[0]["next"] == want and seg[0]["bump"] and (1 << (seg[0]["width"] - 1)) == want, (a, seg[0])   # numpy's stream changed: search a again

# ---- uniform noise, two frames: table-full clears inside segments, every width, all 256 boxes, a ragged last segment -------------------------
info = _add("noise", np.random.default_rng(2).integers(0, 256, (2, 128, 130, 3)), duration_ms=70)
for f in info:
    assert f["boxes"] == 256 and len(f["segments"]) == 3 and 128 * 130 % R.SEGMENT == 256
    assert sum(s["clears"] for s in f["segments"]) >= 1
    assert set().union(*(s["widths"] for s in f["segments"])) == {9, 10, 11, 12}

# ---- flat: one bin with more than 65535 pixels, one box, 255 unused palette entries, 11 segments of pure runs ---------------------------------
info = _add("flat", np.broadcast_to(np.array([200, 31, 97], np.uint8), (300, 300, 3)))
assert info[0]["boxes"] == 1 and len(info[0]["segments"]) == 11 and not info[0]["palette"][1:].any()
assert all(s["clears"] == 0 and s["next"] < 512 for s in info[0]["segments"])

# ---- few colours, odd sizes: at most 256 occupied bins, so median cut splits down to single bins and stops; exact -------------------------------
few = np.random.default_rng(3).integers(0, 6, (3, 37, 53, 3)) * 51
info = _add("few_colours", few, lossless=True, order=R.ping_pong(3), duration_ms=333)
assert all(1 < f["boxes"] <= 216 for f in info)
assert all(f["boxes"] == len(np.unique(fr.reshape(-1, 3), axis=0)) for f, fr in zip(info, few))

# ---- natural statistics --------------------------------------------------------------------------------------------------------------------
info = _add("natural", natural(160, 200))
assert info[0]["boxes"] == 256 and len(info[0]["segments"]) == 4

# ---- a payload of an exact multiple of 255 bytes (no short last sub-block) and of one byte more (a last sub-block of one byte): the natural
# tile trimmed to PAYLOAD_255[k] rows and columns, found by search (scratch/gif_enc_search.py) -------------------------------------------------
PAYLOAD_255 = {0: (40, 28), 1: (35, 32)}
for k, (h, w) in PAYLOAD_255.items():
    info = _add(f"payload_255n_plus{k}", natural(h, w))
    assert info[0]["payload"] % 255 == k and info[0]["payload"] > 255, (k, info[0]["payload"])          # the quantiser or LZW changed: search again

# ---- T = 1, 2, 3 in ping-pong order; no loop extension; a non-contiguous view -----------------------------------------------------------------
for t in (1, 2, 3):
    _add(f"ping_pong_t{t}", np.stack([natural(9, 11, (5 * i, 7 * i)) for i in range(t)]), order=R.ping_pong(t), duration_ms=1000 // t)
assert R.ping_pong(1) == [0] and R.ping_pong(2) == [0, 1] and R.ping_pong(3) == [0, 1, 2, 1] and R.ping_pong(5) == [0, 1, 2, 3, 4, 3, 2, 1]
_add("no_loop", np.stack([natural(20, 31), natural(20, 31, (3, 3))]), loop=None, duration_ms=45)
_add("strided_view", natural(64, 96).reshape(2, 32, 96, 3), view=(slice(None), slice(3, 30, 2), slice(5, 91, 3)), loop=7)
assert not frames("strided_view").flags["C_CONTIGUOUS"] and frames("strided_view").shape == (2, 14, 29, 3)


def dump(out):
    """NAME.in (int32 T, h, w, delay_cs, then the frames) and NAME.want (int32 block bytes, then the block, per frame) for
    scratch/gif_enc_emu.cpp."""
    os.makedirs(out, exist_ok=True)
    for name, c in CASES.items():
        f = np.ascontiguousarray(frames(name))
        t, h, w = f.shape[:3]
        with open(os.path.join(out, name + ".in"), "wb") as fh:
            fh.write(struct.pack("<iiii", t, h, w, c.duration_ms // 10) + f.tobytes())
        with open(os.path.join(out, name + ".want"), "wb") as fh:
            for fr in f:
                blk = R.image_block(fr, c.duration_ms // 10)[0]
                fh.write(struct.pack("<i", len(blk)) + blk)
    return len(CASES)
