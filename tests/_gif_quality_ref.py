"""numpy restatement of the GIF encoder's quality options (csrc/gif_enc.hip, wu_gif_enc_encode_ex): exact palettes, nearest-colour mapping,
ordered dither and one palette for the whole animation.  The median cut, the LZW and the framing are those of tests/_gif_enc_ref.py, imported;
everything else is restated here.  ``encode`` returns the bytes ``wu.gif_enc.GPUGifEncoder(mapping=, dither=, exact=, palette=).encode`` returns;
with no option it returns ``_gif_enc_ref.encode``'s.

All rules are integer:
  exact    at most 256 distinct 24-bit colours (under a global palette: over all frames): the palette is those colours in ascending order of
           r << 16 | g << 8 | b, zeros behind; the index of a pixel is the rank of its colour; no median cut, no dither.  More: the median cut.
  nearest  the index is the entry among 0 .. entries in use - 1 at the smallest squared Euclidean distance in 8-bit RGB (lowest index among equals).
  ordered  the colour searched is clamp(pixel_c + floor((2 M(x, y) + 1 - 64) A_c / 128), 0, 255), M the 8 x 8 threshold of the pixel's position in
           the frame, A_c = min(16, 8 (hi_c - lo_c + 1)) from the final tight 5-bit bounds of the box of the pixel's histogram bin.
  global   one histogram, one median cut or one exact set over all frames; a 256-entry global colour table in the header, no local tables.
"""
import struct

import numpy as np

import _gif_enc_ref as R

NEAREST, ORDERED, EXACT, GLOBAL = 1, 2, 4, 8
BLOCK_FIXED_GLOBAL = 8 + 10 + 1
MAX_PIXELS_GLOBAL = (1 << 32) - 1
MAX_AMPLITUDE = 16


def flags_of(mapping="box", dither=None, exact=False, palette="local"):
    if mapping not in ("box", "nearest") or dither not in (None, "ordered") or palette not in ("local", "global") or not isinstance(exact, bool):
        raise ValueError(f"gif: bad options mapping={mapping!r} dither={dither!r} exact={exact!r} palette={palette!r}")
    if dither == "ordered" and mapping != "nearest":
        raise ValueError("gif: dither='ordered' requires mapping='nearest'")
    return (NEAREST if mapping == "nearest" else 0) | (ORDERED if dither else 0) | (EXACT if exact else 0) | (GLOBAL if palette == "global" else 0)


def block_stride(h, w, flags=0):
    n = R.block_stride(h, w)
    return n - (R.BLOCK_FIXED - BLOCK_FIXED_GLOBAL) if n and flags & GLOBAL else n


def threshold(x, y):
    """M(x, y) of the 8 x 8 ordered dither, 0 .. 63; x and y any integer arrays."""
    x, y = np.asarray(x, np.int64) & 7, np.asarray(y, np.int64) & 7
    m = np.zeros(np.broadcast(x, y).shape, np.int64)
    for b in range(3):
        xb, yb = (x >> b) & 1, (y >> b) & 1
        m += (((xb ^ yb) << 1) | yb) << (2 * (2 - b))
    return m


def colour_keys(px):
    px = np.asarray(px).reshape(-1, 3).astype(np.int64)
    return (px[:, 0] << 16) | (px[:, 1] << 8) | px[:, 2]


def bins_of(px):
    px = np.asarray(px).reshape(-1, 3).astype(np.int64)
    return ((px[:, 0] >> 3) << 10) | ((px[:, 1] >> 3) << 5) | (px[:, 2] >> 3)


def nearest_index(px, palette, n):
    """Brute force: for every pixel of px (N, 3) the lowest index among the first n palette entries at the smallest squared distance."""
    px = np.asarray(px).reshape(-1, 3).astype(np.int64)
    pal = palette[:n].astype(np.int64)
    out = np.empty(len(px), np.uint8)
    for at in range(0, len(px), 4096):
        d = ((px[at:at + 4096, None, :] - pal[None, :, :]) ** 2).sum(2)
        out[at:at + 4096] = np.argmin(d, 1)                                # argmin: the first of equals
    return out


def quantise_group(frames, flags):
    """(palette (256, 3) uint8, index (T, h, w) uint8, entries in use, exact) of frames (T, h, w, 3) that share one palette."""
    t, h, w = frames.shape[:3]
    flat = np.ascontiguousarray(frames).reshape(-1, 3)
    if flags & EXACT:
        keys = colour_keys(flat)
        distinct = np.unique(keys)                                          # ascending
        if len(distinct) <= 256:
            palette = np.zeros((256, 3), np.uint8)
            palette[:len(distinct)] = np.stack([distinct >> 16, (distinct >> 8) & 255, distinct & 255], 1)
            return palette, np.searchsorted(distinct, keys).astype(np.uint8).reshape(t, h, w), len(distinct), True
    palette, box, n = R.quantise(flat.reshape(t * h, w, 3))                # one histogram, one median cut over all pixels of the group
    box = box.reshape(-1)
    if not flags & NEAREST:
        return palette, box.reshape(t, h, w), n, False
    px = flat.astype(np.int64)
    if flags & ORDERED:
        bins = bins_of(flat)
        coord = np.stack([bins >> 10, (bins >> 5) & 31, bins & 31], 1)
        amp = np.zeros((256, 3), np.int64)
        for i in range(n):                                                  # the final tight bounds of a box: those of its occupied bins
            mine = coord[box == i]
            amp[i] = np.minimum(MAX_AMPLITUDE, 8 * (mine.max(0) - mine.min(0) + 1))
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        m = np.tile(threshold(xx, yy).reshape(-1), t)                       # the position in the frame
        off = ((2 * m + 1 - 64)[:, None] * amp[box]) // 128                 # floor
        px = np.clip(px + off, 0, 255)
    return palette, nearest_index(px, palette, n).reshape(t, h, w), n, False


def image_block(palette, index, delay_cs, local):
    h, w = index.shape
    payload, stats = R.lzw(index)
    out = bytearray(b"\x21\xF9\x04\x04" + struct.pack("<H", delay_cs) + b"\x00\x00")
    out += b"\x2C\x00\x00\x00\x00" + struct.pack("<HH", w, h) + (b"\x87" if local else b"\x00")
    if local:
        out += palette.tobytes()
    out += b"\x08"
    for at in range(0, len(payload), 255):
        chunk = payload[at:at + 255]
        out += bytes([len(chunk)]) + chunk
    out += b"\x00"
    return bytes(out), stats, len(payload)


def header(h, w, loop, palette=None):
    """Logical screen descriptor: without a palette that of _gif_enc_ref (0x70), with one a 256-entry global colour table (0xF7)."""
    if palette is None:
        return R.header(h, w, loop)
    out = b"GIF89a" + struct.pack("<HH", w, h) + b"\xF7\x00\x00" + palette.tobytes()
    if loop is not None:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    return out


def encode(frames, duration_ms, loop=0, order=None, mapping="box", dither=None, exact=False, palette="local", stats=False):
    """The file; with ``stats`` also per frame {"palette", "index", "entries", "exact", "payload"}."""
    flags = flags_of(mapping, dither, exact, palette)
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.dtype != np.uint8 or frames.shape[3] != 3 or frames.shape[0] < 1 or R.block_stride(*frames.shape[1:3]) == 0:
        raise ValueError(f"gif: cannot encode {frames.shape} {frames.dtype}")
    t, h, w = frames.shape[:3]
    if flags & GLOBAL and t * h * w > MAX_PIXELS_GLOBAL:
        raise ValueError("gif: too many pixels for one palette")
    order = list(range(t)) if order is None else [int(i) for i in order]
    groups = [quantise_group(frames, flags)] if flags & GLOBAL else [quantise_group(frames[i:i + 1], flags) for i in range(t)]
    done = []
    for i in range(t):
        pal, idx, n, ex = groups[0] if flags & GLOBAL else groups[i]
        idx = idx[i] if flags & GLOBAL else idx[0]
        blk, seg, payload = image_block(pal, idx, duration_ms // 10, not flags & GLOBAL)
        done.append((blk, {"palette": pal, "index": idx, "entries": n, "exact": ex, "payload": payload, "segments": seg}))
    data = header(h, w, loop, groups[0][0] if flags & GLOBAL else None) + b"".join(done[i][0] for i in order) + b"\x3B"
    return (data, [d[1] for d in done]) if stats else data


def lowpass(a):
    """5-tap binomial low-pass (1 4 6 4 1) / 16 along both axes, edges replicated; float64."""
    a = np.asarray(a, np.float64)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for axis in (0, 1):
        pad = [(2, 2) if i == axis else (0, 0) for i in range(a.ndim)]
        p = np.pad(a, pad, mode="edge")
        a = sum(k[j] * np.take(p, np.arange(j, j + a.shape[axis]), axis=axis) for j in range(5))
    return a


def psnr(a, b):
    return R.psnr(a, b)


def psnr_lowpassed(a, b):
    return R.psnr(lowpass(a), lowpass(b))
