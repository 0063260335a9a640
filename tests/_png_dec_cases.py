"""Fixtures of the PNG decoder's device stage, shared by tests/test_gpu_png_dec.py, tests/test_png_dec_glue_cpu.py and the CPU emulation
(scratch/png_dec_emu_fixtures.py writes them to disk for scratch/png_dec_emu.cpp).  Every file is in the segmented framing the parser
accepts; what is inside the segments comes from zlib (``zlib.compressobj(..., wbits=-15)`` per 32 KiB segment) or, where zlib cannot be
made to emit a construct, from the small deflate writer below.  Hand-written streams are single-row images: the first inflated byte is
the filter type, every other byte is free.

``CASES``: name -> Case(file, group, want).  ``want`` is a status name for corrupt files (fixed here, from the rules of the format) and
None for files that must decode; ``expected(name)`` gives (verdict, pixels) of the restatement tests/_png_dec_ref.py, computed once.
"""
import io
import struct
import zlib
from collections import namedtuple

import numpy as np

import _png_dec_ref as D
import _png_enc_ref as E

Case = namedtuple("Case", "file group want")
SEGMENT = D.SEGMENT


# ---- a deflate writer for what zlib never emits ------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _len_symbol(ln):
    i = max(k for k in range(29) if D.LEN_BASE[k] <= ln and (ln < 258 or k == 28))
    return 257 + i, ln - D.LEN_BASE[i], D.LEN_EXTRA[i]


def _dist_symbol(d):
    i = max(k for k in range(30) if D.DIST_BASE[k] <= d)
    return i, d - D.DIST_BASE[i], D.DIST_EXTRA[i]


def simulate(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def lits(data):
    return [("lit", b) for b in data]


def lengths_for(tokens, nlen=None, ndist=None):
    """Code lengths that fit the tokens: Huffman lengths of their histogram; one used distance code gets length 1, none leaves a single
    zero length -- the two degenerate sets RFC 1951 allows."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if t[0] == "lit":
            lf[t[1]] += 1
        else:
            lf[_len_symbol(t[1])[0]] += 1
            df[_dist_symbol(t[2])[0]] += 1
    nlen = nlen or max(257, max(i for i, f in enumerate(lf) if f) + 1)
    lit = E.code_lengths(lf, 15)[:nlen]
    used = [i for i, f in enumerate(df) if f]
    if not used:
        dist = [0]
    elif len(used) == 1:
        dist = [0] * used[0] + [1]
    else:
        dist = E.code_lengths(df, 15)[:max(used) + 1]
    if ndist:
        dist = dist + [0] * (ndist - len(dist))
    return lit, dist


def write_dynamic(bw, final, lit_lens, dist_lens, tokens, end=True):
    """One dynamic-Huffman block.  The lengths need not be a valid set (corrupt headers); then pass no tokens and end=False."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    bw.put(final, 1)
    bw.put(2, 2)
    bw.put(len(lit_lens) - 257, 5)
    bw.put(len(dist_lens) - 1, 5)
    toks = E.length_tokens(lit_lens + dist_lens)
    clfreq = [0] * 19
    for s, _ in toks:
        clfreq[s] += 1
    if sum(1 for f in clfreq if f) == 1:                  # the code-length code itself must be complete: a second symbol, never sent
        clfreq[1 if clfreq[0] else 0] += 1
    cllens = E.code_lengths(clfreq, 7)
    clcodes = E.canonical_codes(cllens)
    ncl = 19
    while ncl > 4 and cllens[E.CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    bw.put(ncl - 4, 4)
    for k in range(ncl):
        bw.put(cllens[E.CL_ORDER[k]], 3)
    for s, e in toks:
        bw.put(clcodes[s], cllens[s])
        if s >= 16:
            bw.put(e, E.CL_EXTRA[s])
    if not tokens and not end:
        return
    lc, dc = E.canonical_codes(lit_lens), E.canonical_codes(dist_lens)
    for t in tokens:
        if t[0] == "lit":
            assert lit_lens[t[1]]
            bw.put(lc[t[1]], lit_lens[t[1]])
        else:
            s, ev, eb = _len_symbol(t[1])
            assert lit_lens[s]
            bw.put(lc[s], lit_lens[s])
            bw.put(ev, eb)
            s, ev, eb = _dist_symbol(t[2])
            assert dist_lens[s]
            bw.put(dc[s], dist_lens[s])
            bw.put(ev, eb)
    if end:
        bw.put(lc[256], lit_lens[256])


def dynamic_stream(tokens, lit_lens=None, dist_lens=None):
    """One final dynamic block of ``tokens``."""
    a, b = lengths_for(tokens)
    bw = BitWriter()
    write_dynamic(bw, 1, lit_lens or a, dist_lens or b, tokens)
    return bw.bytes()


def row_file(stream, inflated):
    """The single-row image whose filtered stream is ``inflated`` (filter type first), with ``stream`` as its one segment."""
    assert len(inflated) % 3 == 1 and len(inflated) <= SEGMENT and inflated[0] <= 4
    return E.frame(1, (len(inflated) - 1) // 3, [stream], zlib.adler32(inflated))


def token_file(tokens, **kw):
    return row_file(dynamic_stream(tokens, **kw), simulate(tokens))


# ---- reading block headers back (the assertions the issue asks for) -----------------------------------------------------------------------------
def dynamic_header(br):
    """tests/_png_dec_ref._dynamic, keeping what it throws away: (literal/length lengths, distance lengths, code-length symbols used)."""
    nlen, ndist, ncode = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
    cl = [0] * 19
    for i in range(ncode):
        cl[E.CL_ORDER[i]] = br.take(3)
    code = D._Code(cl, False)
    lens, used = [], set()
    while len(lens) < nlen + ndist:
        sym = code.decode(br)
        used.add(sym)
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1]] * (3 + br.take(2))
        elif sym == 17:
            lens += [0] * (3 + br.take(3))
        else:
            lens += [0] * (11 + br.take(7))
    return lens[:nlen], lens[nlen:], used


def blocks(body):
    """[{"type", "lit", "dist", "cl_symbols"}] of a valid raw deflate stream (one segment's data)."""
    br, out, n = D._Bits(body), [], 0
    while True:
        final, btype = br.take(1), br.take(2)
        info = {"type": btype, "lit": None, "dist": None, "cl_symbols": set()}
        if btype == 0:
            br.align()
            ln, _ = br.take(16), br.take(16)
            p = br.bytepos()
            br = D._Bits(body)
            br.i = p + ln
            n += ln
            info["empty"] = ln == 0
        else:
            if btype == 2:
                info["lit"], info["dist"], info["cl_symbols"] = dynamic_header(br)
                lit, dist = D._Code(info["lit"], True), D._Code(info["dist"], True)
            else:
                lit, dist = D._fixed()
            while True:
                sym = lit.decode(br)
                if sym == 256:
                    break
                if sym > 256:
                    br.take(D.LEN_EXTRA[sym - 257])
                    br.take(D.DIST_EXTRA[dist.decode(br)])
        out.append(info)
        if final or br.bitpos() == 8 * len(body):
            return out


def segments(data):
    """The raw deflate data of every segment of a file: IDAT bodies without zlib header and Adler-32."""
    info = D.parse(data)
    assert info["supported"], info["reason"]
    n = len(info["idat"])
    return [data[off + (2 if k == 0 else 0):off + ln - (4 if k == n - 1 else 0)] for k, (off, ln) in enumerate(info["idat"])]


def file_blocks(data):
    return [b for seg in segments(data) for b in blocks(seg)]


# ---- images --------------------------------------------------------------------------------------------------------------------------------
def image_file(h, w, content="natural", seed=0, types=None, **kw):
    """(file, rgb): filter types per row given (default: type y % 5), so nothing goes through the byte-by-byte filter chooser."""
    img = E.make_image(h, w, content, seed=seed)
    return D.build(img, filters=types if types is not None else [y % 5 for y in range(h)], **kw), img


def skewed_image(h, w, seed=7):
    """Byte values with a geometric histogram: value k about 2^-(k+1) of the bytes, down to single occurrences."""
    n = h * w * 3
    vals = []
    for k in range(24):
        vals += [k] * max(1, n >> (k + 1))
    vals = (vals + [0] * n)[:n]
    rng = np.random.default_rng(seed)
    return rng.permutation(np.array(vals, np.uint8)).reshape(h, w, 3)


def mixed_block_file(h=40, w=50):
    """One segment holding stored, fixed and dynamic blocks and the empty stored blocks of two full flushes: three compressors, each on
    its own part of the stream, the first two flushed to a byte boundary."""
    img = E.make_image(h, w, "natural", seed=5)
    filtered = D.filter_rows_with(img, [y % 5 for y in range(h)])
    assert len(filtered) <= SEGMENT
    a, b = len(filtered) // 3, 2 * len(filtered) // 3
    c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
    c1 = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    c2 = zlib.compressobj(9, zlib.DEFLATED, -15)
    stream = (c0.compress(filtered[:a]) + c0.flush(zlib.Z_FULL_FLUSH) + c1.compress(filtered[a:b]) + c1.flush(zlib.Z_FULL_FLUSH)
              + c2.compress(filtered[b:]) + c2.flush(zlib.Z_FINISH))
    return E.frame(h, w, [stream], zlib.adler32(filtered)), img


ALLOWED_161718 = [v for v in range(256) if not (20 <= v < 32 or 40 <= v < 45)]


def repeat_symbols_file():
    """A header whose code-length sequence needs all of 16, 17 and 18: 254 literals of 8 bits and four codes of 9 bits, with a run of 12
    and a run of 5 unused literals in between."""
    lit = [8] * 20 + [0] * 12 + [8] * 8 + [0] * 5 + [8] * (254 - 28) + [9] * 4         # 275 symbols; 256 is an 8-bit code
    assert len(lit) == 275 and lit[256] == 8
    rng = np.random.default_rng(11)
    data = bytes([0]) + bytes(rng.choice(np.array(ALLOWED_161718, np.uint8), 3 * 40).tolist())
    tokens = lits(data[:61]) + [("match", 30, 2), ("match", 27, 1)] + lits(data[61:64])        # length symbols 271 (27..30), distance codes 0 and 1
    inflated = simulate(tokens)
    return row_file(dynamic_stream(tokens, lit_lens=lit, dist_lens=[1, 1]), inflated)


def match_file():
    """Distances 1, 2 and 3 with length 258, a distance larger than its length, and a match that starts at byte 0 of the segment."""
    t = lits(b"\x00a") + [("match", 258, 1)] + lits(b"xy") + [("match", 258, 2)] + lits(b"pqr") + [("match", 258, 3)]
    t += [("match", 10, 300)] + lits(b"Z")
    n = len(simulate(t))
    t += [("match", 40, n)]                                                # from byte 0 (the filter type) on
    t += lits(b"w" * ((1 - len(simulate(t))) % 3))
    return token_file(t)


def _flip(data, at, mask=1):
    b = bytearray(data)
    b[at] ^= mask
    return bytes(b)


def _idat(data):
    return [(i, at, ln) for i, (at, kind, ln) in enumerate(D.chunks(data)) if kind == b"IDAT"]


def _raw_row(stream, w=1, adler=1):
    return E.frame(1, w, [stream], adler)


def _build():
    c = {}

    def ok(name, group, file):
        c[name] = Case(file, group, None)

    def bad(name, file, want):
        c[name] = Case(file, "corrupt", want)

    # edge geometry, each as stored, fixed and dynamic blocks
    for h, w in [(1, 1), (1, 7), (9, 1), (6, 2), (105, 104), (128, 85)]:
        for group, kw in (("stored", {"level": 0}), ("fixed", {"strategy": zlib.Z_FIXED}), ("dynamic", {})):
            ok(f"{group}_{h}x{w}", group, image_file(h, w, "natural" if h * w > 64 else "gradient_noise", seed=h, **kw)[0])
    ok("dynamic_long_codes", "dynamic", D.build(skewed_image(30, 100), strategy=zlib.Z_HUFFMAN_ONLY, filters=[0] * 30))
    ok("dynamic_repeat_symbols", "dynamic", repeat_symbols_file())
    ok("dynamic_one_distance_code", "dynamic", token_file(lits(b"\x00abc") + [("match", 258, 1)] + lits(b"def")))
    ok("dynamic_no_distance_code", "dynamic", token_file(lits(b"\x00" + bytes(range(30, 60)))))
    ok("dynamic_matches", "dynamic", match_file())
    ok("dynamic_encoder_75x100", "dynamic", E.encode(E.make_image(75, 100, "gradient_noise")))
    ok("mixed_blocks", "rest", mixed_block_file()[0])
    ok("filters_65x4", "rest", image_file(65, 4, "gradient_noise", 1)[0])                                  # row 64: Paeth
    ok("filters_130x3", "rest", image_file(130, 3, "gradient_noise", 2, [(y + 3) % 5 for y in range(130)])[0])     # row 64: Up, 128: Sub
    ok("filters_130x5", "rest", image_file(130, 5, "gradient_noise", 3, [(y + 4) % 5 for y in range(130)])[0])     # row 64: Average, 128: Up

    # corrupt files
    good, _ = image_file(105, 104)
    ids = _idat(good)
    _, at0, ln0 = ids[0]
    bad("corrupt_chunk_crc", _flip(good, at0 + 8 + ln0 + 1, 0x40), "chunk-crc")
    i1, at1, ln1 = ids[-1]
    body = good[at1 + 8:at1 + 8 + ln1]
    bad("corrupt_adler", D.rechunk(good, i1, _flip(body, len(body) - 1)), "adler")
    bad("corrupt_distance", row_file(dynamic_stream(lits(b"\x00") + [("match", 3, 5)]), b"\0" * 4), "distance")
    bw = BitWriter()
    write_dynamic(bw, 1, [1, 1, 1] + [0] * 253 + [1], [0], [], end=False)
    bad("corrupt_oversubscribed", _raw_row(bw.bytes() + b"\0" * 4), "bad-stream")
    bw = BitWriter()
    write_dynamic(bw, 1, [2, 2] + [0] * 254 + [2], [0], [], end=False)
    bad("corrupt_incomplete", _raw_row(bw.bytes() + b"\0" * 4), "bad-stream")
    bw = BitWriter()
    write_dynamic(bw, 1, [1, 1] + [0] * 255, [0], [], end=False)
    bad("corrupt_no_end_of_block", _raw_row(bw.bytes() + b"\0" * 4), "bad-stream")
    bad("corrupt_block_type_3", _raw_row(b"\x07\0\0\0"), "bad-stream")
    bad("corrupt_stored_nlen", _raw_row(b"\x01\x04\x00\xfb\xfe" + b"\0" * 4, adler=zlib.adler32(b"\0" * 4)), "bad-stream")
    img = E.make_image(6, 5, "gradient_noise")
    filtered = D.filter_rows_with(img, [0, 1, 2, 3, 4, 0])
    for name, data in (("corrupt_one_byte_short", filtered[:-1]), ("corrupt_one_byte_long", filtered + b"\0")):
        bad(name, E.frame(6, 5, D.deflate_pieces(data), zlib.adler32(data)), "segment-size")
    small, _ = image_file(20, 30)
    i, at, ln = _idat(small)[0]
    bad("corrupt_truncated", D.rechunk(small, i, small[at + 8:at + 8 + ln - 12] + small[at + 8 + ln - 4:at + 8 + ln]), "bad-stream")
    f5 = bytearray(filtered)
    f5[2 * 16] = 5
    bad("corrupt_filter_type_5", E.frame(6, 5, D.deflate_pieces(bytes(f5)), zlib.adler32(bytes(f5))), "filter-type")
    return c


CASES = _build()
GROUPS = ("stored", "fixed", "dynamic", "corrupt", "rest")
_EXPECTED = {}


def names(group):
    return [n for n, c in CASES.items() if c.group == group]


def expected(name):
    """(verdict, pixels or None) of the restatement for a case, computed once."""
    if name not in _EXPECTED:
        _EXPECTED[name] = D.decode(CASES[name].file)
    return _EXPECTED[name]


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def non_native_file(h=12, w=17):
    """A palette PNG from Pillow: the parser refuses it (colour type 3)."""
    from PIL import Image
    img = E.make_image(h, w, "gradient", seed=9)
    buf = io.BytesIO()
    Image.fromarray(img).convert("P", palette=Image.ADAPTIVE, colors=16).save(buf, "PNG")
    return buf.getvalue()


# ---- the workspace layout of wu_png_dec_workspace_bytes, restated --------------------------------------------------------------------------------
def workspace_bytes(n, hmax, wmax, n_segments):
    def a256(v):
        return (v + 255) // 256 * 256
    if n <= 0 or hmax <= 0 or wmax <= 0 or hmax > 65535 or wmax > 65535 or n_segments < 0 or n_segments > 0x7FFFFFFF:
        return 0
    flen = hmax * (1 + 3 * wmax)
    nseg = -(-flen // SEGMENT)
    if flen >= 1 << 30 or flen * n >= 1 << 36 or n_segments > n * nseg:
        return 0
    filt = a256(n * a256(nseg * SEGMENT))                 # the filtered streams, whole segments per image
    return filt + a256(max(n_segments, 1) * 16)           # four words per segment: status, two Adler-32 sums, the stored Adler-32
