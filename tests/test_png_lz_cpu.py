"""CPU: the specification of the PNG encoder's LZ77 mode.  tests/_png_lz_ref.py restates the kernels' rule; here that restatement is
held against what it must satisfy whatever the kernels do: Pillow, zlib and the independent inflate of tests/_png_dec_ref.py decode its
files to the input, every token stays inside its segment, no file is larger than the literal-only one, and the size stays near zlib
level 6 on the same segments."""
import io
import zlib

import numpy as np
import pytest

import _png_dec_ref as D
import _png_enc_ref as R
import _png_lz_cases as C
import _png_lz_ref as L

# File size over zlib level 6 (raw deflate, every segment on its own, same framing), measured per case in which at least one segment
# takes the LZ77 block (profiles/png_enc_bench.md): between 0.8946 and 1.2275.  The worst is the 40 x 64 clipped ramp, 232 bytes
# against 189: with so few tokens the greedy parse and the nearest-candidate rule show.  The bar is the worst measured ratio plus 2 %,
# the margin tests/test_png_enc_cpu.py uses for inputs outside the grid.
WORST_MEASURED_RATIO = 1.2276
RATIO_BOUND = WORST_MEASURED_RATIO + 0.02


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_decodes_everywhere_to_the_input(name):
    from PIL import Image
    img, st, _ = C.computed(name)
    data = st["file"]
    Image.open(io.BytesIO(data)).verify()                              # every chunk's CRC
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)    # ... and zlib's inflate with the Adler-32
    h, w, raw = R.unpack(data)                                         # CRCs again, layout, Adler-32
    assert (h, w) == img.shape[:2] and raw == st["filtered"]
    verdict, pixels = D.decode(data)                                   # the independent inflate, segment by segment
    assert verdict == "ok" and np.array_equal(pixels, img)
    # every segment is a deflate stream of its own that ends on a byte boundary and references nothing in front of it
    bodies = [b for k, b in R.parse_chunks(data) if k == b"IDAT"]
    assert len(bodies) == len(st["pieces"])
    bodies[0] = bodies[0][2:]
    bodies[-1] = bodies[-1][:-4]
    for i, (body, piece) in enumerate(zip(bodies, st["pieces"])):
        d = zlib.decompressobj(-15)
        out = d.decompress(body)
        last = i == len(bodies) - 1
        assert out == piece and d.eof == last and not d.unused_data, (name, i)
        assert body == st["segments"][i]


@pytest.mark.parametrize("name", C.NAMES)
def test_never_larger_than_literal_only_and_equal_without_matches(name):
    img, st, lit = C.computed(name)
    assert len(st["file"]) <= len(lit) <= R.out_stride(*img.shape[:2])
    base = R.stages(img)
    for seg, mode, was, stored in zip(st["segments"], st["modes"], base["segments"], base["stored"]):
        if mode == L.LZ77:
            assert len(seg) < len(was)                                 # strictly: a tie keeps the earlier block
        else:
            assert seg == was and mode == (L.STORED if stored else L.LITERAL)
    if name in C.NO_MATCH:
        assert st["file"] == lit and L.LZ77 not in st["modes"]


@pytest.mark.parametrize("name", C.NAMES)
def test_tokens_stay_inside_their_segment(name):
    _, st, _ = C.computed(name)
    for piece, toks in zip(st["pieces"], st["tokens"]):
        at = 0
        for p, ln, d in toks:
            assert p == at
            if ln:
                assert 3 <= ln <= 258 and 1 <= d <= p and p + ln <= len(piece)
                assert piece[p:p + ln] == bytes(piece[p - d + i % d] for i in range(ln))
            at += max(ln, 1)
        assert at == len(piece)


def test_cases_reach_what_they_are_named_for():
    tok = {n: C.computed(n)[1]["tokens"] for n in C.NAMES}
    modes = {n: C.computed(n)[1]["modes"] for n in C.NAMES}
    lens = lambda n: [ln for seg in tok[n] for _, ln, _ in seg if ln]            # noqa: E731
    dists = lambda n: {d for seg in tok[n] for _, ln, d in seg if ln}            # noqa: E731
    assert len(C.computed("99x110_gradient_noise")[1]["pieces"][1]) == 1
    assert {1, 3, 49} & dists("16x16_flat") and modes["16x16_flat"] == [L.LZ77]
    one_row = lens("1x300_flat")                                   # 901 bytes: type byte, one pixel, then a run at distance 3
    assert one_row.count(258) == 3 and 258 > one_row[-1] >= 3 and L.length_symbol(258) == (285, 0, 0) and L.length_symbol(257) == (284, 5, 30)
    assert len(C.computed("128x85_flat")[1]["filtered"]) == R.SEGMENT and modes["128x85_flat"] == [L.LZ77]
    p, ln, d = [t for t in tok["128x85_flat"][0] if t[1]][-1]
    assert p + ln == R.SEGMENT                                      # a run that meets the segment end
    second = tok["128x86_flat"][1]
    assert len(modes["128x86_flat"]) == 2 and second[0][1] == 0 and all(d <= p for p, ln, d in second if ln)
    copied = [(p, ln, d) for p, ln, d in tok["102x100_noise_rows_copied"][0] if d == 30100]
    assert copied and max(ln for _, ln, _ in copied) == 258 and L.dist_symbol(30100) == (29, 13, 5523) and modes["102x100_noise_rows_copied"] == [L.LZ77]
    assert len({L.dist_symbol(d)[0] for d in dists("grid_3x3_of_24")}) >= 10 and any(ln == 0 for _, ln, _ in tok["grid_3x3_of_24"][0])
    assert {193 - 3, 193, 193 + 3} & dists("40x64_ramp_clipped") and modes["40x64_ramp_clipped"] == [L.LZ77]
    small = lens("8x8_saturated")
    assert small and min(small) == 3 and max(small) <= 10 + 10     # short matches at small distances; literal-only wins or ties there
    assert len(modes["200x300_natural"]) == 6 and L.LZ77 in modes["200x300_natural"]
    every = {m for n in C.NAMES for m in modes[n]}
    assert every == {L.STORED, L.LITERAL, L.LZ77}


def _expand(tokens_in):
    """(data, tokens) of a hand-made parse: [("lit", bytes) | ("match", len, dist)] expanded as inflate would."""
    data, toks = bytearray(), []
    for t in tokens_in:
        if t[0] == "lit":
            for b in t[1]:
                toks.append((len(data), 0, 0))
                data.append(b)
        else:
            _, ln, d = t
            assert 1 <= d <= len(data)
            toks.append((len(data), ln, d))
            for _ in range(ln):
                data.append(data[-d])
    return bytes(data), toks


def test_two_alphabet_header_on_hand_made_frequencies():
    """The distance side of the header where an image hardly gets: exactly one distance symbol in use (one code of length 1, an
    incomplete code RFC 1951 allows), only symbol 29 in use (HDIST = 30 with 29 zero lengths in front), and Fibonacci-like counts over
    20 distance symbols, whose Huffman depth of 19 makes the 15-bit fold run on the DISTANCE code -- that branch is hard to reach from
    an image, so it is pinned here only.  Each block must inflate in zlib to the bytes it was made from."""
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, 25000, dtype=np.uint8).tobytes()
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    hand = [("lit", noise[:1100])]
    for sym, count in enumerate(fib):
        hand += [("match", 3 + sym % 4, L.DIST_BASE[sym])] * count
    cases = {
        "one distance symbol": [("lit", noise[:40]), ("match", 5, 7), ("match", 258, 8), ("lit", b"xyz"), ("match", 11, 7)],
        "only symbol 29": [("lit", noise), ("match", 30, 24577), ("match", 4, 24999)],
        "fibonacci over 20 distance symbols": hand,
    }
    for what, tokens_in in cases.items():
        data, toks = _expand(tokens_in)
        dfreq = [0] * 30
        for _, ln, d in toks:
            if ln:
                dfreq[L.dist_symbol(d)[0]] += 1
        lfreq = [0] * 286
        lfreq[256] = 1
        for p, ln, _ in toks:
            lfreq[L.length_symbol(ln)[0] if ln else data[p]] += 1
        hd = L.block_header(lfreq, dfreq)
        used = [l for l in hd["dlens"] if l]
        if what == "one distance symbol":
            assert sum(1 for f in dfreq if f) == 1 and sorted(used) == [1]
        for last in (True, False):
            block = L.lz_block(data, toks, last)
            d = zlib.decompressobj(-15)
            assert d.decompress(block) == data and d.eof == last and not d.unused_data, what
        if what == "only symbol 29":
            assert hd["hdist"] == 30 and hd["dlens"] == [0] * 29 + [1]
        if what.startswith("fibonacci"):
            assert sum(1 for f in dfreq if f) == 20 and max(used) == 15 and sum(2.0 ** -l for l in used) == 1.0
            assert hd["hdist"] == 20
        assert hd["hlit"] == max(257, max(s for s in range(286) if lfreq[s]) + 1)


def test_one_distance_symbol_header_is_one_code_of_length_one():
    data, toks = _expand([("lit", b"abcdefgh"), ("match", 5, 7), ("match", 258, 8), ("match", 11, 7)])
    dfreq = [0] * 30
    for _, ln, d in toks:
        if ln:
            dfreq[L.dist_symbol(d)[0]] += 1
    assert [s for s in range(30) if dfreq[s]] == [5]                  # distances 7 and 8 share symbol 5
    lfreq = [1] * 257 + [0] * 29
    hd = L.block_header(lfreq, dfreq)
    assert hd["dlens"] == [0] * 5 + [1] + [0] * 24 and hd["hdist"] == 6 and hd["hlit"] == 257
    none = L.block_header(lfreq, [0] * 30)                             # no distance at all: the literal-only block's single code
    assert none["dlens"][0] == 1 and none["hdist"] == 1
    assert none["bits"] == 3 + 5 + 5 + 4 + 3 * none["ncl"] + sum(none["cllens"][s] + R.CL_EXTRA.get(s, 0) for s, _ in none["toks"])


@pytest.mark.parametrize("name", C.NAMES)
def test_size_against_zlib_level_6(name):
    img, st, lit = C.computed(name)
    h, w = img.shape[:2]
    z6 = L.zlib6_file(h, w, st["filtered"])
    ratio = len(st["file"]) / z6
    print(f"{name}: literal-only {len(lit)}, lz77 {len(st['file'])}, zlib 6 {z6}, ratio {ratio:.4f}, modes {st['modes']}")
    if L.LZ77 in st["modes"]:
        assert ratio <= RATIO_BOUND


def test_symbol_tables_follow_rfc_1951():
    for length in range(3, 259):
        s, nb, ev = L.length_symbol(length)
        assert 257 <= s <= 285 and L.LEN_BASE[s - 257] + ev == length and 0 <= ev < (1 << nb) or (s, nb, ev) == (285, 0, 0)
    for dist in list(range(1, 600)) + [4096, 4097, 24576, 24577, 30100, 32767]:
        s, nb, ev = L.dist_symbol(dist)
        assert 0 <= s <= 29 and L.DIST_BASE[s] + ev == dist and 0 <= ev < (1 << nb)
    assert (L.LEN_BASE, L.LEN_EXTRA, L.DIST_BASE, L.DIST_EXTRA) == (D.LEN_BASE, D.LEN_EXTRA, D.DIST_BASE, D.DIST_EXTRA)


def test_encoder_option_and_abi_without_a_gpu():
    import ctypes
    from wu import _lib, png_enc
    from wu.png_enc import GPUPngEncoder
    with pytest.raises(ValueError, match="matching"):
        GPUPngEncoder(matching="bogus")
    enc = GPUPngEncoder(device="cuda", matching="lz77")               # constructing needs no GPU
    assert enc.matching == "lz77" and enc.stats["native"] == 0
    enc.close()
    plain = GPUPngEncoder()
    assert plain.matching == "none"
    plain.close()
    lib = _lib.load()
    for n, h, w in ((4, 64, 64), (1, 200, 300), (3, 1, 1)):
        base = lib.wu_png_enc_workspace_bytes(n, h, w)
        nseg = -(-h * (1 + 3 * w) // R.SEGMENT)
        assert lib.wu_png_enc_workspace_bytes_ex(n, h, w, 0) == base
        assert lib.wu_png_enc_workspace_bytes_ex(n, h, w, png_enc.LZ77) == base + n * nseg * R.SEGMENT * 4
        assert 0 < lib.wu_png_enc_seginfo_offset(n, h, w) < base
    assert lib.wu_png_enc_workspace_bytes_ex(4, 64, 64, 2) == 0 and lib.wu_png_enc_workspace_bytes_ex(0, 64, 64, 1) == 0
    one = ctypes.c_void_p(256)           # never dereferenced: every call below fails validation first
    args = dict(src=one, dtype=2, sn=192, sc=1, sy=24, sx=3, desc=one, ws=one, ws_bytes=1 << 30, out=one, out_bytes=1 << 30, result=one,
                N=1, H=8, W=8, flags=1, stream=None)

    def call(**kw):
        return lib.wu_png_enc_encode_ex(*dict(args, **kw).values())
    assert call(flags=2) < 0 and b"flags" in lib.wu_last_error()
    assert call(flags=-1) < 0 and b"flags" in lib.wu_last_error()
    assert call(src=None) < 0 and b"null" in lib.wu_last_error()
    need = lib.wu_png_enc_workspace_bytes_ex(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) < 0 and b"workspace too small" in lib.wu_last_error()
    assert call(flags=0, ws_bytes=lib.wu_png_enc_workspace_bytes(1, 8, 8) - 1) < 0 and b"workspace too small" in lib.wu_last_error()


def test_fullres_cli_has_the_option():
    from wu import fullres
    with pytest.raises(SystemExit) as e:
        fullres.main(["--help"])
    assert e.value.code == 0
    import inspect
    assert "--png-lz77" in inspect.getsource(fullres)
