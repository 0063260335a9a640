"""numpy / pure-Python restatement of the PNG encoder of csrc/png_enc.hip: filter choice, segmentation, code-length construction with
its tie-breaking, the run-length-coded code-length alphabet, LSB-first bit packing, the stored-block decision, checksums and framing.
``encode`` returns the bytes the kernels write.  Also the chunk parser and the independent pieces the tests hold both against
(a vectorised filter heuristic, zlib's Huffman-only stream with the same framing, the stored-block bound).

PNG is lossless, so -- unlike the JPEG encoder -- Pillow's bytes are not the bar (Pillow runs zlib's LZ77 matcher, the kernels do
not): the bar is that the file decodes to the input pixels with every checksum right, and that the kernels equal this file byte for byte.
"""
import os
import struct
import zlib

import numpy as np

SEGMENT = 32768                       # filtered bytes per deflate block (wu_png_enc_segment_bytes)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}
GOLDEN_JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


# ---- test images -----------------------------------------------------------------------------------------------------------------------
def make_image(h, w, content, seed=0):
    """(h, w, 3) uint8; deterministic in its arguments."""
    rng = np.random.default_rng([h, w, seed, sum(content.encode())])
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content in ("gradient", "gradient_noise"):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(h + w - 2, 1)], axis=-1)
        if content == "gradient_noise":
            base = base + rng.normal(0, 6, (h, w, 3))
        return np.clip(base, 0, 255).astype(np.uint8)
    if content == "flat":
        return np.broadcast_to(np.array([200, 31, 97], dtype=np.uint8), (h, w, 3)).copy()
    if content == "saturated":
        return rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255
    if content == "natural":              # the decoded baseline fixture, mirrored and tiled to the size
        from PIL import Image
        a = np.asarray(Image.open(os.path.join(GOLDEN_JPEG, "baseline_420.jpg")).convert("RGB"))
        a = np.concatenate([a, a[:, ::-1]], 1)
        a = np.concatenate([a, a[::-1]], 0)
        return np.tile(a, (-(-h // a.shape[0]), -(-w // a.shape[1]), 1))[:h, :w].copy()
    raise ValueError(content)


# h x w, content: the smallest shapes at which each mechanism can fail.  128 x 85 filters to exactly one segment (128 * 256 bytes),
# 99 x 110 to one segment and one byte (99 * 331 = 32769).
GRID = [(1, 1, "noise"), (5, 7, "gradient"), (1, 33, "gradient_noise"), (33, 1, "gradient_noise"), (16, 16, "flat"), (8, 8, "saturated"),
        (64, 64, "noise"), (75, 100, "gradient_noise"), (200, 300, "natural"), (128, 85, "gradient_noise"), (99, 110, "gradient_noise")]
COMPRESSIBLE = [c for c in GRID if c[2] != "noise"]


def case_id(case):
    return f"{case[0]}x{case[1]}_{case[2]}"


# ---- filtering ---------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(rgb):
    """The filtered stream, h * (1 + 3 w) bytes, byte by byte as the filter kernel computes it: per row the five residuals (bpp 3, the
    prior row of row 0 is zeros), cost = sum of min(r, 256 - r), the smallest cost, ties to the smallest type."""
    h, w, _ = rgb.shape
    rows = rgb.reshape(h, 3 * w).astype(np.int64)
    out = bytearray()
    zero = [0] * (3 * w)
    for y in range(h):
        cur = rows[y].tolist()
        up = rows[y - 1].tolist() if y else zero
        res = [[], [], [], [], []]
        for i, x in enumerate(cur):
            a = cur[i - 3] if i >= 3 else 0
            b = up[i]
            c = up[i - 3] if i >= 3 else 0
            res[0].append(x)
            res[1].append((x - a) & 255)
            res[2].append((x - b) & 255)
            res[3].append((x - ((a + b) >> 1)) & 255)
            res[4].append((x - _paeth(a, b, c)) & 255)
        costs = [sum(min(r, 256 - r) for r in rr) for rr in res]
        best = costs.index(min(costs))
        out.append(best)
        out += bytes(res[best])
    return bytes(out)


def filter_types_vectorised(rgb):
    """The chosen filter type per row, written independently of ``filter_rows``: whole-image numpy arithmetic."""
    h, w, _ = rgb.shape
    x = rgb.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) % 256
    cost = np.minimum(res, 256 - res).sum(axis=2)             # (5, h)
    return np.argmin(cost, axis=0)                            # first minimum: the smallest type


# ---- Huffman codes -------------------------------------------------------------------------------------------------------------------------
def code_lengths(freq, maxbits):
    """Length per symbol (0: unused).  Symbols in use sorted by (count, symbol); Huffman's algorithm on two queues, a leaf winning a tie
    against an internal node; the number of codes per length from the tree, lengths over ``maxbits`` folded back as zlib's gen_bitlen
    does; the lengths then go to the symbols in sorted order, longest first."""
    order = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    m = len(order)
    lens = [0] * len(freq)
    blc = [0] * 16
    if m == 1:
        blc[1] = 1
    elif m > 1:
        wt = [freq[s] for s in order] + [0] * (m - 1)
        parent = [0] * (2 * m - 1)
        i, j = 0, m
        for k in range(m, 2 * m - 1):
            pick = []
            for _ in range(2):
                if i < m and (j >= k or wt[i] <= wt[j]):
                    pick.append(i)
                    i += 1
                else:
                    pick.append(j)
                    j += 1
            wt[k] = wt[pick[0]] + wt[pick[1]]
            parent[pick[0]] = parent[pick[1]] = k
        depth = [0] * (2 * m - 1)
        for k in range(2 * m - 3, m - 1, -1):
            depth[k] = depth[parent[k]] + 1
        overflow = sum(1 for k in range(m, 2 * m - 2) if depth[k] > maxbits)       # gen_bitlen counts internal nodes too
        for leaf in range(m):
            d = depth[parent[leaf]] + 1
            if d > maxbits:
                d = maxbits
                overflow += 1
            blc[d] += 1
        while overflow > 0:
            bits = maxbits - 1
            while blc[bits] == 0:
                bits -= 1
            blc[bits] -= 1
            blc[bits + 1] += 2
            blc[maxbits] -= 1
            overflow -= 2
    i = 0
    for b in range(maxbits, 0, -1):
        for _ in range(blc[b]):
            lens[order[i]] = b
            i += 1
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2, each code bit-reversed (Huffman codes enter the LSB-first stream starting from their most significant bit)."""
    blc = [0] * 17
    for l in lens:
        blc[l] += 1
    blc[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + blc[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(int(format(nxt[l], f"0{l}b")[::-1], 2))
            nxt[l] += 1
        else:
            out.append(0)
    return out


def length_tokens(seq):
    """(symbol, extra value) of the code-length alphabet for a sequence of code lengths: 18 = 11..138 zeros, 17 = 3..10 zeros,
    16 = the previous length 3..6 times more; greedy, longest first."""
    toks, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                c = min(run, 138)
                toks.append((18, c - 11))
                run -= c
            if run >= 3:
                toks.append((17, run - 3))
                run = 0
            toks += [(0, 0)] * run
        else:
            toks.append((v, 0))
            run -= 1
            while run >= 3:
                c = min(run, 6)
                toks.append((16, c - 3))
                run -= c
            toks += [(v, 0)] * run
    return toks


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self, nbytes):
        return self.acc.to_bytes(nbytes, "little")


def deflate_segment(data, last):
    """One segment of the filtered stream -> (bytes, stored).  A literal-only dynamic-Huffman block (257 literal/length codes, one
    distance code of length 1), closed -- unless it is the last -- by an empty stored block that pads to a byte boundary; or one stored
    block where that is not larger."""
    freq = np.bincount(np.frombuffer(data, np.uint8), minlength=257).tolist()
    freq[256] = 1
    lens = code_lengths(freq, 15)
    codes = canonical_codes(lens)
    toks = length_tokens(lens + [1])
    clfreq = [0] * 19
    for s, _ in toks:
        clfreq[s] += 1
    cllens = code_lengths(clfreq, 7)
    clcodes = canonical_codes(cllens)
    ncl = 19
    while ncl > 4 and cllens[CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    hdr_bits = 3 + 5 + 5 + 4 + 3 * ncl + sum(cllens[s] + CL_EXTRA.get(s, 0) for s, _ in toks)
    total = hdr_bits + sum(f * l for f, l in zip(freq[:256], lens)) + lens[256]
    dyn = (total + 7) // 8 if last else (total + 3 + 7) // 8 + 4
    if len(data) + 5 <= dyn:
        n = len(data)
        return bytes([1 if last else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + data, True
    bw = _Bits()
    bw.put(1 if last else 0, 1)
    bw.put(2, 2)
    bw.put(0, 5)
    bw.put(0, 5)
    bw.put(ncl - 4, 4)
    for k in range(ncl):
        bw.put(cllens[CL_ORDER[k]], 3)
    for s, e in toks:
        bw.put(clcodes[s], cllens[s])
        if s >= 16:
            bw.put(e, CL_EXTRA[s])
    assert bw.n == hdr_bits
    # the literals, vectorised: bit b of every code at its offset
    sym = np.frombuffer(data, np.uint8)
    ln = np.array(lens[:256], np.int64)[sym]
    cd = np.array(codes[:256], np.int64)[sym]
    off = hdr_bits + np.concatenate([[0], np.cumsum(ln)[:-1]])
    bits = np.zeros(dyn * 8, np.uint8)
    for b in range(15):
        sel = ln > b
        bits[off[sel] + b] = (cd[sel] >> b) & 1
    lit = int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")
    bw.acc |= lit
    bw.n = total - lens[256]
    bw.put(codes[256], lens[256])
    assert bw.n == total
    if not last:
        bw.put(0, 3)
        bw.n = (bw.n + 7) // 8 * 8
        bw.put(0xFFFF0000, 32)
    return bw.bytes(dyn), False


# ---- framing -------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def ihdr(h, w):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))


def frame(h, w, segments, adler):
    """Signature, IHDR, one IDAT per deflate segment (zlib header 78 01 in the first, Adler-32 in the last), IEND."""
    out = [SIGNATURE, ihdr(h, w)]
    for i, s in enumerate(segments):
        out.append(chunk(b"IDAT", (b"\x78\x01" if i == 0 else b"") + s + (struct.pack(">I", adler) if i == len(segments) - 1 else b"")))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def stages(rgb):
    rgb = np.ascontiguousarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w, _ = rgb.shape
    filt = filter_rows(rgb)
    pieces = [filt[i:i + SEGMENT] for i in range(0, len(filt), SEGMENT)]
    segs = [deflate_segment(p, i == len(pieces) - 1) for i, p in enumerate(pieces)]
    return {"filtered": filt, "segments": [s for s, _ in segs], "stored": [st for _, st in segs],
            "file": frame(h, w, [s for s, _ in segs], zlib.adler32(filt))}


def encode(rgb):
    """The file csrc/png_enc.hip writes for an (h, w, 3) uint8 image."""
    return stages(rgb)["file"]


def out_stride(h, w):
    """The exact worst case of an h x w file -- every segment a stored block: what wu_png_enc_out_stride returns."""
    n = h * (1 + 3 * w)
    nseg = -(-n // SEGMENT)
    return n + 5 * nseg + 12 * nseg + len(SIGNATURE) + 25 + 2 + 4 + 12


def huffman_only_file(h, w, filtered):
    """zlib's own Huffman-only stream of the same filtered bytes (level 6, memLevel 9) in the same framing, cut at the same places:
    the size the kernels' files are held against."""
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    z = co.compress(filtered) + co.flush()
    nseg = -(-len(filtered) // SEGMENT)
    return len(SIGNATURE) + 25 + 12 * nseg + len(z) + 12


# ---- the tests' parser ---------------------------------------------------------------------------------------------------------------------
def parse_chunks(data):
    """[(type, body)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert len(body) == n and zlib.crc32(kind + body) == crc, f"chunk {kind!r} at {at}: bad CRC"
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1][0] == b"IEND"
    return out


def unpack(data):
    """(h, w, filtered stream) of a file of this encoder: parses, checks the layout, inflates (zlib checks the Adler-32)."""
    chunks = parse_chunks(data)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"} and chunks[-1][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    z = b"".join(b for k, b in chunks if k == b"IDAT")
    assert z[:2] == b"\x78\x01"
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and not d.unused_data
    return h, w, raw
