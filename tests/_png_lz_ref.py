"""Pure-Python / numpy restatement of the PNG encoder's opt-in LZ77 mode (csrc/png_enc.hip, ``WU_PNG_ENC_LZ77``;
``GPUPngEncoder(matching="lz77")``).  Filters, code construction, framing and the stored / literal-only blocks are ``_png_enc_ref``'s,
unchanged; this file adds, per 32 KiB segment of the filtered stream (nothing crosses a segment):

The match array.  ``rowstride = 1 + 3 w``.  Position p (p + 3 <= n) has the hash ``((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1 mod 2^32)
>> 19`` of its three bytes (13 bits).  The segment is walked in blocks of 64 positions; every position of a block first READS the head
table at its hash, then the whole block is inserted (the largest position of a hash wins, which is what ``atomicMax`` gives in any
order).  So the head candidate of p is the nearest position with p's hash in front of p's block -- never one of p's own block.  The
candidates of p, in this order: the distances 1, 3, rowstride - 3, rowstride, rowstride + 3, then the head candidate; one with a
distance outside [1, p] is skipped.  Each is extended while the bytes agree, to at most ``min(258, n - p)``.  The longest wins, a tie
goes to the EARLIER candidate of the list, and a length under 3 is no match: ``(0, 0)``.

One lazy step, on the array as it was found: the match at p is dropped, (0, 0), where the match at p + 1 is longer.

The parse: greedy from position 0 -- a match where the array has one, else a literal -- so ``next[p] = p + max(len, 1)``.

The block: one dynamic-Huffman block of the tokens.  Literal/length frequencies (end-of-block counted once) and distance frequencies
each go through ``code_lengths(., 15)``; no distance in use gives one distance code of length 1, as in the literal-only block, and a
single distance in use gets length 1 (RFC 1951 3.2.7).  HLIT and HDIST are trimmed to the last used code (at least 257 and 1); the
HLIT + HDIST lengths are run-length coded as ONE sequence with ``length_tokens`` and the code-length code is built as in the
literal-only block.  Length and distance codes are followed by their extra bits.  Closing empty stored block as before.

The selection: the smallest of stored, literal-only and LZ77; a tie goes to the earlier of that order.  Hence a segment without a
match is today's, a file is never larger than today's, and ``out_stride`` stays the exact worst case.
"""
import zlib

import numpy as np

import _png_enc_ref as R

BLOCK = 64                       # positions that read the head table before any of them is inserted
HASH_BITS = 13
MIN_MATCH, MAX_MATCH = 3, 258
# RFC 1951 3.2.5
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
STORED, LITERAL, LZ77 = 1, 0, 2            # a segment's mode, as the kernels record it (word 3 of the segment info)


def length_symbol(length):
    """(symbol 257..285, extra bits, extra value)"""
    k = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def dist_symbol(dist):
    """(symbol 0..29, extra bits, extra value)"""
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


def _hashes(x):
    v = x[:-2].astype(np.uint64) | (x[1:-1].astype(np.uint64) << np.uint64(8)) | (x[2:].astype(np.uint64) << np.uint64(16))
    return (((v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64).tolist()


def head_candidates(data):
    """Per position the head candidate (-1: none)."""
    n = len(data)
    cand = [-1] * n
    if n < 3:
        return cand
    hs = _hashes(np.frombuffer(data, np.uint8))
    head = {}
    for blk in range(0, n - 2, BLOCK):
        hi = min(blk + BLOCK, n - 2)
        for p in range(blk, hi):
            cand[p] = head.get(hs[p], -1)
        for p in range(blk, hi):                 # increasing: the largest position of a hash stays
            head[hs[p]] = p
    return cand


def _common(data, p, c, limit):
    """Bytes that agree from p and c on, at most ``limit``."""
    a, b = data[p:p + limit], data[c:c + limit]
    if a == b:
        return limit
    lo, hi = 0, limit - 1                        # the first difference lies in [0, limit)
    while lo < hi:
        mid = (lo + hi) // 2
        if a[:mid + 1] == b[:mid + 1]:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _run_lengths(x, d):
    """Per position p >= d the number of bytes that agree between p.. and (p - d).., unbounded (0 for p < d)."""
    n = len(x)
    out = np.zeros(n, np.int64)
    if d < 1 or d >= n:
        return out
    eq = x[d:] == x[:-d]                         # eq[i]: byte d + i equals byte i
    idx = np.arange(len(eq))
    stop = np.where(~eq, idx, len(eq))           # the next index >= i at which they differ
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    out[d:] = stop - idx
    return out


def matches(data, rowstride):
    """[(len, dist)] per position of one segment; (0, 0) where there is no match."""
    n = len(data)
    x = np.frombuffer(data, np.uint8)
    limit = np.minimum(MAX_MATCH, n - np.arange(n))
    best = np.zeros(n, np.int64)
    bdist = np.zeros(n, np.int64)
    for d in (1, 3, rowstride - 3, rowstride, rowstride + 3):
        ln = np.minimum(_run_lengths(x, d), limit)
        ln[ln < MIN_MATCH] = 0
        take = ln > best                         # strictly longer: a tie stays with the earlier candidate
        best[take], bdist[take] = ln[take], d
    best, bdist = best.tolist(), bdist.tolist()
    cand = head_candidates(data)
    for p in range(n):
        c = cand[p]
        if c >= 0 and data[c:c + 3] == data[p:p + 3] and p + 3 <= n:
            ln = _common(data, p, c, min(MAX_MATCH, n - p))
            if ln >= MIN_MATCH and ln > best[p]:
                best[p], bdist[p] = ln, p - c
    found = list(zip(best, bdist))
    return [(0, 0) if ln and p + 1 < n and found[p + 1][0] > ln else (ln, d) for p, (ln, d) in enumerate(found)]


def greedy_tokens(data, match):
    """[(position, len, dist)]: len 0 is the literal data[position]."""
    toks, p = [], 0
    while p < len(data):
        ln, d = match[p]
        toks.append((p, ln, d))
        p += max(ln, 1)
    return toks


def block_header(lfreq, dfreq):
    """The two codes and the header of a dynamic block from the frequencies of the 286 literal/length symbols (end-of-block included)
    and the 30 distance symbols: dict with llens, dlens (286 / 30 lengths), hlit, hdist, cllens, ncl, toks, bits (of the header)."""
    llens = R.code_lengths(list(lfreq), 15)
    dlens = R.code_lengths(list(dfreq), 15) if any(dfreq) else [1] + [0] * 29
    hlit = max(257, max(s for s in range(286) if llens[s]) + 1)
    hdist = max(1, max(s for s in range(30) if dlens[s]) + 1)
    toks = R.length_tokens(llens[:hlit] + dlens[:hdist])
    clfreq = [0] * 19
    for s, _ in toks:
        clfreq[s] += 1
    cllens = R.code_lengths(clfreq, 7)
    ncl = 19
    while ncl > 4 and cllens[R.CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    bits = 3 + 5 + 5 + 4 + 3 * ncl + sum(cllens[s] + R.CL_EXTRA.get(s, 0) for s, _ in toks)
    return {"llens": llens, "dlens": dlens, "hlit": hlit, "hdist": hdist, "cllens": cllens, "ncl": ncl, "toks": toks, "bits": bits}


def put_header(bw, hd, last):
    clcodes = R.canonical_codes(hd["cllens"])
    bw.put(1 if last else 0, 1)
    bw.put(2, 2)
    bw.put(hd["hlit"] - 257, 5)
    bw.put(hd["hdist"] - 1, 5)
    bw.put(hd["ncl"] - 4, 4)
    for k in range(hd["ncl"]):
        bw.put(hd["cllens"][R.CL_ORDER[k]], 3)
    for s, e in hd["toks"]:
        bw.put(clcodes[s], hd["cllens"][s])
        if s >= 16:
            bw.put(e, R.CL_EXTRA[s])


def lz_block(data, toks, last):
    """The LZ77 block of a segment's tokens, closed like the literal-only one."""
    lfreq, dfreq = [0] * 286, [0] * 30
    lfreq[256] = 1
    for p, ln, d in toks:
        if ln:
            lfreq[length_symbol(ln)[0]] += 1
            dfreq[dist_symbol(d)[0]] += 1
        else:
            lfreq[data[p]] += 1
    hd = block_header(lfreq, dfreq)
    lcodes, dcodes = R.canonical_codes(hd["llens"]), R.canonical_codes(hd["dlens"])
    bw = R._Bits()
    put_header(bw, hd, last)
    assert bw.n == hd["bits"]
    for p, ln, d in toks:
        if ln:
            s, nb, ev = length_symbol(ln)
            bw.put(lcodes[s], hd["llens"][s])
            bw.put(ev, nb)
            s, nb, ev = dist_symbol(d)
            bw.put(dcodes[s], hd["dlens"][s])
            bw.put(ev, nb)
        else:
            bw.put(lcodes[data[p]], hd["llens"][data[p]])
    bw.put(lcodes[256], hd["llens"][256])
    if not last:
        bw.put(0, 3)
        bw.n = (bw.n + 7) // 8 * 8
        bw.put(0xFFFF0000, 32)
    nbytes = (bw.n + 7) // 8
    return bw.bytes(nbytes)


def deflate_segment(data, last, rowstride):
    """(bytes, mode, tokens): today's segment unless the LZ77 block is strictly smaller."""
    base, stored = R.deflate_segment(data, last)
    toks = greedy_tokens(data, matches(data, rowstride))
    lz = lz_block(data, toks, last)
    if len(lz) < len(base):
        return lz, LZ77, toks
    return base, STORED if stored else LITERAL, toks


def stages(rgb):
    rgb = np.ascontiguousarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w, _ = rgb.shape
    filt = R.filter_rows(rgb)
    pieces = [filt[i:i + R.SEGMENT] for i in range(0, len(filt), R.SEGMENT)]
    segs = [deflate_segment(p, i == len(pieces) - 1, 1 + 3 * w) for i, p in enumerate(pieces)]
    return {"filtered": filt, "pieces": pieces, "segments": [s for s, _, _ in segs], "modes": [m for _, m, _ in segs],
            "tokens": [t for _, _, t in segs], "file": R.frame(h, w, [s for s, _, _ in segs], zlib.adler32(filt))}


def encode(rgb):
    """The file csrc/png_enc.hip writes for an (h, w, 3) uint8 image with WU_PNG_ENC_LZ77."""
    return stages(rgb)["file"]


def zlib6_file(h, w, filtered):
    """zlib level 6 (raw deflate, each segment on its own, sync-flushed like the encoder's) in the same framing: the size reference."""
    pieces = [filtered[i:i + R.SEGMENT] for i in range(0, len(filtered), R.SEGMENT)]
    segs = []
    for i, p in enumerate(pieces):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        if i == len(pieces) - 1:
            segs.append(co.compress(p) + co.flush())
        else:
            segs.append(co.compress(p) + co.flush(zlib.Z_FULL_FLUSH))
    return len(R.frame(h, w, segs, zlib.adler32(filtered)))
