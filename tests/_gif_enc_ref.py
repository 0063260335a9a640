"""numpy / pure-Python restatement of the GIF encoder of csrc/gif_enc.hip: the 32768-bin histogram, median cut with its tie-breaking, the
rounded-mean palette, the bin -> index map, the segmented LZW with its width rule at segment ends, LSB-first bit packing, sub-blocks and
framing.  ``encode`` returns the bytes ``wu.gif_enc.GPUGifEncoder.encode`` returns.

A GIF is a palette image, so Pillow's bytes are not the bar (Pillow orders its palette differently and runs one unsegmented LZW): the bar is
that Pillow decodes every frame to ``palette[index]`` with the right frame count, duration and loop, that the quantiser is no worse than
Pillow's own, and that the kernels equal this file byte for byte.

Documented limitation: the index of a pixel is the box of its 5-bit-per-channel histogram bin, so an image with several distinct colours in
one bin is not reproduced exactly even if it has 256 colours or fewer.
"""
import struct

import numpy as np

SEGMENT = 8192                        # indices per LZW segment (wu_gif_enc_segment_pixels)
CLEAR, EOI, FIRST_CODE, MAX_CODES = 256, 257, 258, 4096
BLOCK_FIXED = 8 + 10 + 768 + 1        # graphic control extension, image descriptor, local colour table, minimum code size
MAX_PIXELS = 1 << 26


def ping_pong(t):
    """[0 .. t-1, t-2 .. 1]: the order demo.py writes its frames in."""
    return list(range(t)) + list(range(t - 2, 0, -1))


def block_stride(h, w):
    """The worst case of an h x w image block: every pixel a 12-bit code, four more codes per segment.  0: cannot be encoded."""
    if h < 1 or w < 1 or h > 65535 or w > 65535 or h * w > MAX_PIXELS:
        return 0
    nseg = -(-h * w // SEGMENT)
    p = (12 * (h * w + 4 * nseg) + 7) // 8
    return BLOCK_FIXED + p + -(-p // 255) + 1


# ---- quantiser ---------------------------------------------------------------------------------------------------------------------------
def quantise(frame):
    """(palette (256, 3) uint8, index (h, w) uint8, boxes in use) of one (h, w, 3) uint8 frame."""
    px = np.ascontiguousarray(frame).reshape(-1, 3).astype(np.int64)
    bins = ((px[:, 0] >> 3) << 10) | ((px[:, 1] >> 3) << 5) | (px[:, 2] >> 3)
    count = np.bincount(bins, minlength=32768)
    sums = np.stack([np.bincount(bins, px[:, c], minlength=32768).astype(np.int64) for c in range(3)], 1)     # float64 weights: exact below 2^53
    occ = np.nonzero(count)[0]
    n_occ = count[occ]
    coord = np.stack([occ >> 10, (occ >> 5) & 31, occ & 31], 1)          # 5-bit bin coordinates, R G B
    box = np.zeros(len(occ), np.int64)
    n = [int(n_occ.sum())]
    lo = [coord.min(0)]
    hi = [coord.max(0)]
    while len(n) < 256:
        best, best_score = -1, 0
        for i in range(len(n)):
            ext = int((hi[i] - lo[i]).max())
            if ext > 0 and n[i] * ext > best_score:                        # ties: the lowest box index
                best, best_score = i, n[i] * ext
        if best < 0:
            break
        ext = hi[best] - lo[best]
        axis = int(np.argmax(ext))                                         # ties: R, then G, then B
        mine = box == best
        marg = np.bincount(coord[mine, axis], n_occ[mine], minlength=32).astype(np.int64)
        cum, k = 0, int(lo[best][axis])
        while True:
            cum += int(marg[k])
            if 2 * cum >= n[best]:
                break
            k += 1
        k = min(k, int(hi[best][axis]) - 1)
        moved = mine & (coord[:, axis] > k)
        new = len(n)
        box[moved] = new
        kept = mine & ~moved
        assert moved.any() and kept.any()
        n[best], lo[best], hi[best] = int(n_occ[kept].sum()), coord[kept].min(0), coord[kept].max(0)
        n.append(int(n_occ[moved].sum()))
        lo.append(coord[moved].min(0))
        hi.append(coord[moved].max(0))
    palette = np.zeros((256, 3), np.uint8)
    for i in range(len(n)):
        s = sums[occ[box == i]].sum(0)
        palette[i] = (2 * s + n[i]) // (2 * n[i])
    table = np.zeros(32768, np.uint8)
    table[occ] = box
    return palette, table[bins].reshape(frame.shape[0], frame.shape[1]), len(n)


# ---- LZW ---------------------------------------------------------------------------------------------------------------------------------
def lzw_segment(idx, first, last):
    """(bits as an int, number of bits, stats) of one segment of indices."""
    acc, nbits = 0, 0
    width, nxt, table, clears = 9, FIRST_CODE, {}, 0
    widths = set()

    def emit(code, w):
        nonlocal acc, nbits
        acc |= code << nbits
        nbits += w
        widths.add(w)
    if first:
        emit(CLEAR, 9)
    prefix = int(idx[0])
    for b in idx[1:].tolist():
        key = (prefix << 8) | b
        hit = table.get(key)
        if hit is not None:
            prefix = hit
            continue
        emit(prefix, width)
        if nxt < MAX_CODES:
            table[key] = nxt
            if nxt == (1 << width) and width < 12:
                width += 1
            nxt += 1
        else:
            emit(CLEAR, width)
            table, width, nxt = {}, 9, FIRST_CODE
            clears += 1
        prefix = b
    emit(prefix, width)
    bump = nxt < MAX_CODES and nxt == (1 << width) and width < 12       # the decoder does add one more entry
    if bump:
        width += 1
    emit(EOI if last else CLEAR, width)
    return acc, nbits, {"next": nxt, "width": width, "clears": clears, "bump": bump, "widths": widths, "bits": nbits}


def lzw(index):
    """(payload bytes, per-segment stats) of one frame's row-major index stream."""
    flat = np.ascontiguousarray(index).reshape(-1)
    nseg = -(-len(flat) // SEGMENT)
    acc, nbits, stats = 0, 0, []
    for s in range(nseg):
        a, nb, st = lzw_segment(flat[s * SEGMENT:(s + 1) * SEGMENT], s == 0, s == nseg - 1)
        acc |= a << nbits
        nbits += nb
        stats.append(st)
    return acc.to_bytes((nbits + 7) // 8, "little"), stats


def image_block(frame, delay_cs):
    """(block bytes, info) of one frame: what the device writes per distinct frame."""
    h, w = frame.shape[:2]
    palette, index, boxes = quantise(frame)
    payload, stats = lzw(index)
    out = bytearray(b"\x21\xF9\x04\x04" + struct.pack("<H", delay_cs) + b"\x00\x00")
    out += b"\x2C\x00\x00\x00\x00" + struct.pack("<HH", w, h) + b"\x87"
    out += palette.tobytes() + b"\x08"
    for at in range(0, len(payload), 255):
        chunk = payload[at:at + 255]
        out += bytes([len(chunk)]) + chunk
    out += b"\x00"
    return bytes(out), {"palette": palette, "index": index, "boxes": boxes, "segments": stats, "payload": len(payload)}


def header(h, w, loop):
    out = b"GIF89a" + struct.pack("<HH", w, h) + b"\x70\x00\x00"
    if loop is not None:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    return out


def encode(frames, duration_ms, loop=0, order=None, stats=False):
    """The file of (T, h, w, 3) uint8 frames shown in ``order`` (default 0 .. T-1); with ``stats`` also the per-frame info: palette, index,
    boxes, payload bytes and per segment the final ``next``, the width of the trailing code, the table-full clears and whether the
    end-of-segment bump fired."""
    frames = np.asarray(frames)
    t, h, w = frames.shape[:3]
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or t < 1 or block_stride(h, w) == 0:
        raise ValueError(f"gif: cannot encode {frames.shape} {frames.dtype}")
    order = list(range(t)) if order is None else [int(i) for i in order]
    done = [image_block(f, duration_ms // 10) for f in frames]          # every distinct frame once
    data = header(h, w, loop) + b"".join(done[i][0] for i in order) + b"\x3B"
    return (data, [d[1] for d in done]) if stats else data


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
