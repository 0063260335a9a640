"""The cases of the GIF encoder's quality options (tests/test_gif_quality_cpu.py, tests/test_gpu_gif_quality.py; scratch/gif_enc_emu.cpp
reads them through ``dump``), with the restatement's file and stats per option set computed once.  Every case is ASSERTED here to reach the edge
it is named for, so a case that stops exercising its edge fails at import instead of passing for nothing."""
import os
import struct
from collections import namedtuple

import numpy as np

import _gif_quality_ref as Q

GOLDEN_JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")

# the option sets every case is run under, and the defaults
OPTIONS = {
    "nearest": dict(mapping="nearest"),
    "nearest_ordered": dict(mapping="nearest", dither="ordered"),
    "exact": dict(exact=True),
    "best": dict(mapping="nearest", dither="ordered", exact=True, palette="global"),
    "global": dict(palette="global"),
}
DEFAULT = dict(mapping="box", dither=None, exact=False, palette="local")

Case = namedtuple("Case", "base view duration_ms loop order")
CASES = {}
_done = {}


def frames(name):
    c = CASES[name]
    return c.base if c.view is None else c.base[c.view]


def expected(name, options):
    """(file, per-frame info) of the restatement for a case under OPTIONS[options] (or "default"), computed once."""
    if (name, options) not in _done:
        c = CASES[name]
        kw = DEFAULT if options == "default" else OPTIONS[options]
        _done[name, options] = Q.encode(frames(name), c.duration_ms, c.loop, c.order, stats=True, **kw)
    return _done[name, options]


def _add(name, base, view=None, duration_ms=100, loop=0, order=None):
    base = np.array(base, dtype=np.uint8, order="C")                     # a writable copy of its own
    if base.ndim == 3:
        base = base[None]
    CASES[name] = Case(base, view, duration_ms, loop, order)


def distinct(a):
    return len(np.unique(Q.colour_keys(a)))


def ramp(h, w):
    """The sky ramp: r = 40 + 120 y/H + 30 x/W, g = 90 + 100 y/H + 20 x/W, b = 200 + 50 y/H - 40 x/W, rounded."""
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    return np.rint(np.stack([40 + 120 * y + 30 * x, 90 + 100 * y + 20 * x, 200 + 50 * y - 40 * x], -1)).astype(np.uint8)


def set_hash(colour):
    """The slot a colour's probe starts at in the device's colour set (csrc/gif_enc.hip set_hash; 1024 slots)."""
    return ((np.asarray(colour, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


SET_SLOTS = 1024

# ---- the grey fixture: 256 colours in 32 bins ----------------------------------------------------------------------------------------------
from PIL import Image                                                       # noqa: E402
grey = np.asarray(Image.open(os.path.join(GOLDEN_JPEG, "grey.png")).convert("RGB"))
_add("grey", grey)
assert distinct(grey) == 256 and len(np.unique(Q.bins_of(grey))) == 32

# ---- exactly 256 colours, four in each of 64 bins; and the same with one pixel changed: 257, the boundary of the exact path ----------------
i = np.concatenate([np.arange(256), np.random.default_rng(0).integers(0, 256, 20 * 24 - 256)])
i = np.random.default_rng(1).permutation(i).reshape(20, 24)
c256 = np.stack([100 + (i & 3), 50 + 9 * ((i >> 2) & 7), 30 + 20 * (i >> 5)], -1).astype(np.uint8)
_add("colours_256", c256)
assert distinct(c256) == 256 and len(np.unique(Q.bins_of(c256))) == 64
c257 = c256.copy()
c257[7, 11] = (3, 250, 128)
_add("colours_257", c257)
assert distinct(c257) == 257

# ---- 1 x 1, and one colour on 5 x 7 ----------------------------------------------------------------------------------------------------------
_add("one_pixel", np.array([[[[9, 250, 77]]]]))
_add("one_colour", np.broadcast_to(np.array([13, 200, 255], np.uint8), (5, 7, 3)))

# ---- the 96 x 128 sky ramp; the same with its lower half uniform noise over the whole colour cube --------------------------------------------
_add("ramp", ramp(96, 128))
assert distinct(ramp(96, 128)) > 256
noisy = ramp(96, 128)
noisy[48:] = np.random.default_rng(2).integers(0, 256, (48, 128, 3))
_add("ramp_half_noise", noisy)

# ---- 96 x 131: the segment boundary (pixel 8192 = row 62, column 70) falls inside a row, and W is no multiple of 8 -------------------------
ragged = ramp(96, 131).astype(np.int64) + np.random.default_rng(3).integers(-2, 3, (96, 131, 3))
_add("ragged_96x131", np.clip(ragged, 0, 255))
assert 8192 % 131 != 0 and 131 % 8 != 0 and 96 * 131 > 8192

# ---- ties: pixels at the same distance from two palette entries in use (the lowest index wins) ------------------------------------------------
# By construction: entries (60, 60, 60) and (70, 60, 60) -- two bins, each the rounded mean of its many pixels -- and 12 pixels of (65, 60, 60),
# which share the second one's bin without moving its mean and lie 5 levels from both; on top, whatever ties a coarse random field gives.
ties = np.random.default_rng(4).integers(0, 40, (40, 52, 3)) * 4 + 60
ties[:24, :24] = np.where(np.random.default_rng(5).random((24, 24, 1)) < 0.5, (60, 60, 60), (70, 60, 60))
ties[np.arange(12) * 2, np.arange(12) * 2] = (65, 60, 60)
_add("ties", ties)


def count_ties(name, options):
    n = 0
    for f, info in zip(frames(name), expected(name, options)[1]):
        pal = info["palette"][:info["entries"]].astype(np.int64)
        d = ((f.reshape(-1, 1, 3).astype(np.int64) - pal[None]) ** 2).sum(2)
        n += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    return n


pal = expected("ties", "nearest")[1][0]["palette"].astype(np.int64)[:expected("ties", "nearest")[1][0]["entries"]]
d = ((np.array([65, 60, 60]) - pal) ** 2).sum(1)
assert (d == d.min()).sum() == 2 and d.min() == 25, np.sort(d)[:3]          # the built pixels are tied between exactly two entries
assert count_ties("ties", "nearest") >= 12, count_ties("ties", "nearest")

# ---- 256 colours that all start their probe at the same slot of the device's colour set, near its end: one probe run of 256 slots that wraps
# round; and a 257th such colour, which the set must count -------------------------------------------------------------------------------------
keys = np.arange(1 << 20)
same = keys[set_hash(keys) == SET_SLOTS - 100][:257]
assert len(same) == 257
collide = np.stack([same >> 16, (same >> 8) & 255, same & 255], -1).astype(np.uint8)
_add("set_collisions_256", np.random.default_rng(5).permutation(collide[:256]).reshape(16, 16, 3))
_add("set_collisions_257", np.concatenate([collide, collide[:3]]).reshape(13, 20, 3))
assert distinct(frames("set_collisions_256")) == 256 and distinct(frames("set_collisions_257")) == 257

# ---- T = 3 with a constant left half -------------------------------------------------------------------------------------------------------------
still = np.stack([ramp(32, 48)] * 3).astype(np.int64)
for t in range(3):
    still[t, :, 24:] = np.clip(still[t, :, 24:] + np.random.default_rng(6 + t).integers(-20, 21, (32, 24, 3)) + 15 * t, 0, 255)
_add("still_left_half_t3", still, order=[0, 1, 2, 1], duration_ms=250)
assert np.array_equal(still[0, :, :24], still[1, :, :24]) and np.array_equal(still[0, :, :24], still[2, :, :24])
assert not np.array_equal(still[0], still[1])

# ---- a non-contiguous view ---------------------------------------------------------------------------------------------------------------------
wide = ramp(64, 96).astype(np.int64) + np.random.default_rng(9).integers(-3, 4, (64, 96, 3))
_add("strided_view", np.clip(wide, 0, 255).reshape(2, 32, 96, 3), view=(slice(None), slice(3, 30, 2), slice(5, 91, 3)), loop=3, duration_ms=80)
assert not frames("strided_view").flags["C_CONTIGUOUS"] and frames("strided_view").shape == (2, 14, 29, 3)


def dump(out):
    """NAME.OPTIONS.in (int32 T, h, w, delay_cs, flags, then the frames) and NAME.OPTIONS.want (768 bytes of the global palette, zeros under local
    ones; then per frame int32 entries, exact, block bytes, and the block) for scratch/gif_enc_emu.cpp."""
    os.makedirs(out, exist_ok=True)
    n = 0
    for name, c in CASES.items():
        f = np.ascontiguousarray(frames(name))
        t, h, w = f.shape[:3]
        for options, kw in OPTIONS.items():
            flags = Q.flags_of(**kw)
            _, info = expected(name, options)
            with open(os.path.join(out, f"{name}.{options}.in"), "wb") as fh:
                fh.write(struct.pack("<iiiii", t, h, w, c.duration_ms // 10, flags) + f.tobytes())
            with open(os.path.join(out, f"{name}.{options}.want"), "wb") as fh:
                fh.write(info[0]["palette"].tobytes() if flags & Q.GLOBAL else bytes(768))
                for fi in info:
                    blk = Q.image_block(fi["palette"], fi["index"], c.duration_ms // 10, not flags & Q.GLOBAL)[0]
                    fh.write(struct.pack("<iii", fi["entries"], int(fi["exact"]), len(blk)) + blk)
            n += 1
    return n
