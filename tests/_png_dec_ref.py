"""Pure-Python restatement of the segmented-PNG decoder: the header parse of csrc/png_dec.hip with its refusal reasons, and what a device
stage has to reproduce -- a bit-serial inflate of one segment with status codes in a fixed order of checks, the Adler-32 / filter-type
verdict, the unfilter -- and the fixture builder: files in the encoder's framing (every 32 KiB of the filtered stream an independent deflate segment in an IDAT
chunk of its own) deflated by zlib itself, so with matches, several blocks per segment, fixed-Huffman and stored blocks.

The bar is zlib and Pillow: ``decode`` must return the pixels Pillow returns for every file it accepts, and must accept nothing
``zlib.decompress`` rejects.
"""
import struct
import zlib

import numpy as np

import _png_enc_ref as E

SEGMENT = E.SEGMENT
MAX_CHUNK = 40960                     # wu_png_dec_max_chunk_bytes
MAX_NATIVE_PIXELS = 89478485
REASONS = {0: "ok", 1: "not-png", 2: "header", 3: "colour-type", 4: "bit-depth", 5: "interlaced", 6: "not-segmented", 7: "too-large",
           8: "corrupt-chunk"}
STATUS = {0: "ok", 1: "chunk-crc", 2: "bad-stream", 3: "distance", 4: "segment-size", 5: "filter-type", 6: "adler"}
OK, CHUNK_CRC, BAD_STREAM, DISTANCE, SEGMENT_SIZE, FILTER_TYPE, ADLER = range(7)

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


# ---- the header parse (wu_png_dec_parse) ---------------------------------------------------------------------------------------------------
def parse(data, max_pixels=MAX_NATIVE_PIXELS):
    """{"supported", "reason" (a name), "h", "w", "n_idat", "n_segments", "idat": [(offset, length)]}."""
    out = {"supported": False, "reason": "ok", "h": 0, "w": 0, "n_idat": 0, "n_segments": 0, "idat": []}

    def refuse(reason):
        out["reason"] = reason
        return out

    n = len(data)
    if n < 8 or data[:8] != E.SIGNATURE:
        return refuse("not-png")
    if n < 33 or data[8:12] != b"\0\0\0\x0d" or data[12:16] != b"IHDR" or zlib.crc32(data[12:29]) != struct.unpack(">I", data[29:33])[0]:
        return refuse("header")
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", data[16:29])
    if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF or comp != 0 or flt != 0 or lace > 1:
        return refuse("header")
    out["h"], out["w"] = h, w
    if colour != 2:
        return refuse("colour-type")
    if depth != 8:
        return refuse("bit-depth")
    if lace != 0:
        return refuse("interlaced")
    if h * w > max_pixels or w > 65535 or h > 65535:
        return refuse("too-large")
    out["n_segments"] = -(-h * (1 + 3 * w) // SEGMENT)
    at, state = 33, 0
    while True:
        if n - at < 12:
            return refuse("corrupt-chunk")
        ln, = struct.unpack(">I", data[at:at + 4])
        if ln > n - at - 12:
            return refuse("corrupt-chunk")
        kind = data[at + 4:at + 8]
        if kind == b"IDAT":
            if state == 2:
                return refuse("corrupt-chunk")
            state = 1
            out["idat"].append((at + 8, ln))
        elif kind == b"IEND":
            break
        else:
            if not kind[0] & 0x20:
                return refuse("corrupt-chunk")
            if state == 1:
                state = 2
        at += 12 + ln
    idat = out["idat"]
    out["n_idat"] = len(idat)
    if not idat:
        return refuse("corrupt-chunk")
    if (len(idat) != out["n_segments"] or any(ln > MAX_CHUNK for _, ln in idat) or idat[0][1] < 2 or idat[-1][1] < 4
            or (len(idat) == 1 and idat[0][1] < 6)):
        return refuse("not-segmented")
    cmf, flg = data[idat[0][0]], data[idat[0][0] + 1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or flg & 0x20:
        return refuse("corrupt-chunk")
    out["supported"] = True
    return out


# ---- inflate of one segment ----------------------------------------------------------------------------------------------------------------
class _Fail(Exception):
    def __init__(self, status):
        super().__init__(STATUS[status])
        self.status = status


class _Bits:
    """LSB-first reader; asking for a bit behind the end is the input running out."""
    def __init__(self, data):
        self.data, self.i, self.acc, self.n = data, 0, 0, 0

    def take(self, n):
        while self.n < n:
            if self.i >= len(self.data):
                raise _Fail(BAD_STREAM)
            self.acc |= self.data[self.i] << self.n
            self.i += 1
            self.n += 8
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.n -= n
        return v

    def align(self):
        self.acc >>= self.n & 7
        self.n -= self.n & 7

    def bytepos(self):                       # only when aligned
        return self.i - self.n // 8

    def bitpos(self):
        return 8 * self.i - self.n


class _Code:
    """Canonical Huffman code from its lengths, validated as zlib's inflate_table validates: over-subscribed sets are refused, incomplete
    ones too unless ``single_ok`` and the set is one code of length 1 (or empty)."""
    def __init__(self, lens, single_ok):
        self.cnt = [0] * 16
        for l in lens:
            self.cnt[l] += 1
        self.cnt[0] = 0
        left = 1
        for b in range(1, 16):
            left = 2 * left - self.cnt[b]
            if left < 0:
                raise _Fail(BAD_STREAM)
        if left > 0 and not (single_ok and max(lens) <= 1):
            raise _Fail(BAD_STREAM)
        self.sorted = [s for l in range(1, 16) for s in range(len(lens)) if lens[s] == l]

    def decode(self, br):
        code = first = index = 0
        for ln in range(1, 16):
            code |= br.take(1)
            c = self.cnt[ln]
            if code - c < first:
                return self.sorted[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise _Fail(BAD_STREAM)


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _Code([5] * 32, False))
    return _FIXED


def _dynamic(br):
    nlen, ndist, ncode = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
    bad = nlen > 286 or ndist > 30
    cl = [0] * 19
    for i in range(ncode):
        cl[E.CL_ORDER[i]] = br.take(3)
    if bad:
        raise _Fail(BAD_STREAM)
    clcode = _Code(cl, False)
    lens = []
    while len(lens) < nlen + ndist:
        sym = clcode.decode(br)
        if sym < 16:
            lens.append(sym)
            continue
        if sym == 16:
            if not lens:
                raise _Fail(BAD_STREAM)
            val, rep = lens[-1], 3 + br.take(2)
        elif sym == 17:
            val, rep = 0, 3 + br.take(3)
        else:
            val, rep = 0, 11 + br.take(7)
        if len(lens) + rep > nlen + ndist:
            raise _Fail(BAD_STREAM)
        lens += [val] * rep
    if lens[256] == 0:
        raise _Fail(BAD_STREAM)
    return _Code(lens[:nlen], True), _Code(lens[nlen:], True)


def inflate_segment(body, expected, last):
    """One segment's deflate data (the IDAT body without the zlib header of the first; with the Adler-32 of the last) ->
    (status, bytes produced, stored Adler-32 or None)."""
    br = _Bits(body)
    out = bytearray()
    try:
        while True:
            bfinal, btype = br.take(1), br.take(2)
            if btype == 3 or (bfinal and not last):
                raise _Fail(BAD_STREAM)
            if btype == 0:
                br.align()
                ln, nln = br.take(16), br.take(16)
                p = br.bytepos()
                if ln ^ 0xFFFF != nln or p + ln > len(body):
                    raise _Fail(BAD_STREAM)
                if len(out) + ln > expected:
                    raise _Fail(SEGMENT_SIZE)
                out += body[p:p + ln]
                br = _Bits(body)
                br.i = p + ln
            else:
                lit, dist = _fixed() if btype == 1 else _dynamic(br)
                while True:
                    sym = lit.decode(br)
                    if sym > 285:
                        raise _Fail(BAD_STREAM)
                    if sym < 256:
                        if len(out) >= expected:
                            raise _Fail(SEGMENT_SIZE)
                        out.append(sym)
                        continue
                    if sym == 256:
                        break
                    ln = LEN_BASE[sym - 257] + br.take(LEN_EXTRA[sym - 257])
                    ds = dist.decode(br)
                    if ds > 29:
                        raise _Fail(BAD_STREAM)
                    d = DIST_BASE[ds] + br.take(DIST_EXTRA[ds])
                    if d > len(out):
                        raise _Fail(DISTANCE)
                    if len(out) + ln > expected:
                        raise _Fail(SEGMENT_SIZE)
                    for _ in range(ln):
                        out.append(out[-d])
            if bfinal:
                p = (br.bitpos() + 7) // 8
                if len(body) - p != 4:
                    raise _Fail(BAD_STREAM)
                if len(out) != expected:
                    raise _Fail(SEGMENT_SIZE)
                return OK, bytes(out), struct.unpack(">I", body[p:p + 4])[0]
            if br.bitpos() == 8 * len(body):
                if last:
                    raise _Fail(BAD_STREAM)
                if len(out) != expected:
                    raise _Fail(SEGMENT_SIZE)
                return OK, bytes(out), None
    except _Fail as f:
        return f.status, bytes(out), None


# ---- unfilter ------------------------------------------------------------------------------------------------------------------------------
def unfilter(filtered, h, w):
    """(h, w, 3) uint8 from the filtered stream; bpp = 3, the prior row of row 0 is zeros.  Filter bytes are 0..4 here."""
    row = 1 + 3 * w
    prev = [0] * (3 * w)
    out = bytearray()
    for y in range(h):
        ft = filtered[y * row]
        x = filtered[y * row + 1:(y + 1) * row]
        cur = [0] * (3 * w)
        for i in range(3 * w):
            a = cur[i - 3] if i >= 3 else 0
            b = prev[i]
            c = prev[i - 3] if i >= 3 else 0
            pred = (0, a, b, (a + b) >> 1, E._paeth(a, b, c))[ft]
            cur[i] = (x[i] + pred) & 255
        out += bytes(cur)
        prev = cur
    return np.frombuffer(bytes(out), np.uint8).reshape(h, w, 3)


def decode(data, max_pixels=MAX_NATIVE_PIXELS):
    """(verdict, pixels): verdict is "ok" (pixels an (h, w, 3) uint8 array), a parser reason or a device status (pixels None)."""
    info = parse(data, max_pixels)
    if not info["supported"]:
        return info["reason"], None
    h, w, nseg = info["h"], info["w"], info["n_segments"]
    total = h * (1 + 3 * w)
    pieces, stored = [], None
    for k, (off, ln) in enumerate(info["idat"]):
        crc, = struct.unpack(">I", data[off + ln:off + ln + 4])
        if zlib.crc32(data[off - 4:off + ln]) != crc:
            return STATUS[CHUNK_CRC], None
        body = data[off + (2 if k == 0 else 0):off + ln]
        st, piece, adler = inflate_segment(body, min(SEGMENT, total - k * SEGMENT), k == nseg - 1)
        if st != OK:
            return STATUS[st], None
        pieces.append(piece)
        stored = adler
    filtered = b"".join(pieces)
    row = 1 + 3 * w
    if any(filtered[y * row] > 4 for y in range(h)):
        return STATUS[FILTER_TYPE], None
    if zlib.adler32(filtered) != stored:
        return STATUS[ADLER], None
    return "ok", unfilter(filtered, h, w)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
def filter_rows_with(rgb, filters):
    """The filtered stream with the given filter type per row."""
    h, w, _ = rgb.shape
    assert len(filters) == h
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
    res = (np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) % 256).astype(np.uint8)
    return b"".join(bytes([t]) + res[t, y].tobytes() for y, t in enumerate(filters))


def deflate_pieces(filtered, level=6, mem_level=8, strategy=0, flush=zlib.Z_FULL_FLUSH):
    """The 32 KiB pieces of ``filtered`` through ONE raw deflate stream, flushed between the pieces."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    pieces = [filtered[i:i + SEGMENT] for i in range(0, len(filtered), SEGMENT)]
    return [co.compress(p) + co.flush(zlib.Z_FINISH if i == len(pieces) - 1 else flush) for i, p in enumerate(pieces)]


_FILTERED = {}


def encoder_filtered(rgb):
    """E.filter_rows(rgb), computed once per image (it is a byte-by-byte Python loop)."""
    key = (rgb.shape, rgb.tobytes())
    if key not in _FILTERED:
        _FILTERED[key] = E.filter_rows(rgb)
    return _FILTERED[key]


def build(rgb, level=6, mem_level=8, strategy=0, flush=zlib.Z_FULL_FLUSH, filters=None):
    """A PNG file of ``rgb`` in the encoder's framing, deflated by zlib: the encoder's filter choice, or ``filters`` per row."""
    rgb = np.ascontiguousarray(rgb)
    h, w, _ = rgb.shape
    filtered = encoder_filtered(rgb) if filters is None else filter_rows_with(rgb, filters)
    return E.frame(h, w, deflate_pieces(filtered, level, mem_level, strategy, flush), zlib.adler32(filtered))


# The decoder's cases: E.GRID through zlib in the ways that reach every block type, and forced filter types.  name -> (rgb, file).
ZLIB_VARIANTS = {"zlib6": {}, "mem1": {"mem_level": 1}, "fixed": {"strategy": zlib.Z_FIXED}, "level0": {"level": 0}}
# (h, w, filter type per row): every type on row 0, on middle rows and on width-1 rows; all types next to each other, and across the 64-row
# groups a wave-wide unfilter would take (row 64 is a Paeth row)
FILTER_CASES = ([(7, 9, [t] * 7) for t in range(5)] + [(9, 1, [t] * 9) for t in range(5)]
                + [(7, 9, [(3 * y + 1) % 5 for y in range(7)]), (70, 5, [y % 5 for y in range(70)]), (130, 3, [4 - y % 5 for y in range(130)])])
_FIXTURES = {}


def zlib_fixtures(variant):
    """{case id: (rgb, file)} of E.GRID deflated by zlib with ZLIB_VARIANTS[variant]."""
    if variant not in _FIXTURES:
        _FIXTURES[variant] = {E.case_id(c): (img, build(img, **ZLIB_VARIANTS[variant])) for c in E.GRID for img in [E.make_image(*c)]}
    return _FIXTURES[variant]


def filter_fixtures():
    if "filters" not in _FIXTURES:
        out = {}
        for i, (h, w, types) in enumerate(FILTER_CASES):
            img = E.make_image(h, w, "gradient_noise", seed=i)
            out[f"{h}x{w}_f{'' .join(map(str, types[:7]))}"] = (img, build(img, filters=types))
        _FIXTURES["filters"] = out
    return _FIXTURES["filters"]


def chunks(data):
    """[(offset of the length field, type, body length)] of a well-formed file."""
    at, out = 8, []
    while at < len(data):
        ln, = struct.unpack(">I", data[at:at + 4])
        out.append((at, data[at + 4:at + 8], ln))
        at += 12 + ln
    return out


def rechunk(data, index, body):
    """``data`` with the body of chunk ``index`` replaced and its length and CRC made right."""
    at, kind, ln = chunks(data)[index]
    return data[:at] + E.chunk(kind, body) + data[at + 12 + ln:]


def with_ancillary(data):
    """A tEXt chunk before the IDAT run and a tIME-like private chunk behind it."""
    cs = chunks(data)
    first = next(at for at, kind, _ in cs if kind == b"IDAT")
    iend = next(at for at, kind, _ in cs if kind == b"IEND")
    return data[:first] + E.chunk(b"tEXt", b"Comment\0segmented") + data[first:iend] + E.chunk(b"prVt", b"\1\2\3") + data[iend:]


def corruptions():
    """name -> (file, expected verdict or None where ``decode`` decides): a valid six-segment file with one thing wrong each."""
    big = E.make_image(200, 300, "natural")
    good = build(big)
    cs = [c for c in chunks(good) if c[1] == b"IDAT"]
    at, _, ln = cs[2]
    flipped = bytearray(good)
    flipped[at + 8 + ln // 2] ^= 0x10
    out = {"bit-flip": (bytes(flipped), "chunk-crc")}
    idx = [i for i, c in enumerate(chunks(good)) if c[1] == b"IDAT"]
    out["bit-flip-crc-repaired"] = (rechunk(good, idx[2], bytes(flipped[at + 8:at + 8 + ln])), None)
    at_l, _, ln_l = cs[-1]
    body = bytearray(good[at_l + 8:at_l + 8 + ln_l])
    body[-1] ^= 1
    out["adler"] = (rechunk(good, idx[-1], bytes(body)), "adler")
    filtered = bytearray(encoder_filtered(big))
    filtered[7 * (1 + 3 * 300)] = 5
    out["filter-byte-5"] = (E.frame(200, 300, deflate_pieces(bytes(filtered)), zlib.adler32(bytes(filtered))), "filter-type")
    out["sync-flush"] = (build(big, flush=zlib.Z_SYNC_FLUSH), "distance")
    out["segment-cut-short"] = (rechunk(good, idx[1], good[cs[1][0] + 8:cs[1][0] + 8 + cs[1][2] - 9]), "bad-stream")
    return out
