"""CPU: the PNG decoder's host side.  (1) the restatement tests/_png_dec_ref.py against zlib and Pillow on files of every block type,
with the verdicts it gives for corrupt files held against zlib; (2) wu_png_dec_parse through the C ABI -- good files, ancillary
chunks, every refusal reason, truncations, hostile chunk lengths -- against the restatement's parser."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import _png_dec_ref as D
import _png_enc_ref as E


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _zlib_filtered(data):
    """The filtered stream as zlib inflates the concatenated IDAT bodies (raises zlib.error on anything wrong)."""
    z = b"".join(data[off:off + ln] for off, ln in D.parse(data)["idat"])
    return zlib.decompress(z)


def _save(img, mode=None, **kw):
    buf = io.BytesIO()
    im = Image.fromarray(img)
    (im.convert(mode) if mode else im).save(buf, "PNG", **kw)
    return buf.getvalue()


def _with_ihdr(data, **fields):
    """``data`` with IHDR fields replaced (w, h, depth, colour, comp, flt, lace) and the IHDR CRC made right."""
    names = ("w", "h", "depth", "colour", "comp", "flt", "lace")
    vals = dict(zip(names, struct.unpack(">IIBBBBB", data[16:29])))
    vals.update(fields)
    return data[:8] + E.chunk(b"IHDR", struct.pack(">IIBBBBB", *(vals[k] for k in names))) + data[33:]


SMALL = E.make_image(5, 7, "gradient")
BIG = E.make_image(200, 300, "natural")


# ---- (1) the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(D.ZLIB_VARIANTS))
def test_restatement_decodes_zlib_files(variant):
    for name, (img, data) in D.zlib_fixtures(variant).items():
        verdict, px = D.decode(data)
        assert verdict == "ok", (name, verdict)
        assert np.array_equal(px, img), name
        assert np.array_equal(_pillow(data), img), name
        info = D.parse(data)
        total = img.shape[0] * (1 + 3 * img.shape[1])
        for k, (off, ln) in enumerate(info["idat"]):                      # every segment inflates on its own, with zlib too
            body = data[off + (2 if k == 0 else 0):off + ln - (4 if k == len(info["idat"]) - 1 else 0)]
            assert len(zlib.decompressobj(-15).decompress(body)) == min(D.SEGMENT, total - k * D.SEGMENT), (name, k)


def test_restatement_decodes_encoder_and_filter_files():
    for c in E.GRID:
        img = E.make_image(*c)
        verdict, px = D.decode(E.encode(img))
        assert verdict == "ok" and np.array_equal(px, img), E.case_id(c)
    for name, (img, data) in D.filter_fixtures().items():
        verdict, px = D.decode(data)
        assert verdict == "ok" and np.array_equal(px, img), name
        assert np.array_equal(_pillow(data), img), name


def test_fixtures_reach_every_block_type():
    """What the variants are for: matches (an overlapping one of length 258 in the flat image), several blocks per segment, fixed and
    stored blocks."""
    def first_block_type(body):
        return (body[0] >> 1) & 3

    flat = D.zlib_fixtures("zlib6")["16x16_flat"][1]
    off, ln = D.parse(flat)["idat"][0]
    assert ln < 16 * 49 // 4                                              # only matches compress a flat image that far
    for variant, first in (("fixed", 1), ("level0", 0), ("zlib6", 2)):
        data = D.zlib_fixtures(variant)["75x100_gradient_noise"][1]
        off, ln = D.parse(data)["idat"][0]
        assert first_block_type(data[off + 2:off + ln]) == first, variant
    a = D.zlib_fixtures("mem1")["64x64_noise"][1]
    b = D.zlib_fixtures("zlib6")["64x64_noise"][1]
    assert len(a) != len(b)                                               # memLevel 1 cuts the segment into many blocks


def test_sync_flush_segments_depend_on_their_predecessors():
    data = D.build(BIG, flush=zlib.Z_SYNC_FLUSH)
    assert D.parse(data)["supported"]
    assert D.decode(data)[0] == "distance"
    assert np.array_equal(_pillow(data), BIG)                             # a valid file all the same: Pillow's to decode
    info = D.parse(data)
    dependent = 0
    for k, (off, ln) in enumerate(info["idat"]):
        body = data[off + (2 if k == 0 else 0):off + ln]
        dependent += D.inflate_segment(body, D.SEGMENT, k == len(info["idat"]) - 1)[0] == D.DISTANCE
    assert dependent >= 1


def test_restatement_verdicts_on_corrupt_files():
    for name, (data, want) in D.corruptions().items():
        verdict, _ = D.decode(data)
        assert verdict != "ok", name
        if want is not None:
            assert verdict == want, (name, verdict)
        if name not in ("sync-flush",):                                   # everything else zlib rejects too, or the filter byte is illegal
            if name == "filter-byte-5":
                _zlib_filtered(data)
            elif name != "bit-flip":                                      # (a CRC error is the chunk layer's, not zlib's)
                with pytest.raises(zlib.error):
                    _zlib_filtered(data)


def test_restatement_accepts_nothing_zlib_rejects():
    """Bit flips all over a one-segment file with the chunk CRC repaired, each inflated by zlib too: whatever the restatement accepts zlib
    inflates, to the same bytes; and the flips are not all of one kind (some break the stream, some only the checksum)."""
    img, data = D.zlib_fixtures("zlib6")["75x100_gradient_noise"]
    idx = next(i for i, c in enumerate(D.chunks(data)) if c[1] == b"IDAT")
    at, _, ln = D.chunks(data)[idx]
    rng = np.random.default_rng(5)
    seen, zlib_rejects = set(), 0
    for pos in sorted(set(rng.integers(0, ln, 24).tolist()) | {0, 1, 2, 3, ln - 5, ln - 1}):
        body = bytearray(data[at + 8:at + 8 + ln])
        body[pos] ^= 1 << int(rng.integers(0, 8))
        bad = D.rechunk(data, idx, bytes(body))
        try:
            by_zlib = zlib.decompress(bytes(body))
        except zlib.error:
            by_zlib = None
            zlib_rejects += 1
        info = D.parse(bad)
        if not info["supported"]:                                         # the flip hit the zlib header: the parser's to refuse
            assert info["reason"] == "corrupt-chunk" and pos < 2, pos
            continue
        verdict, px = D.decode(bad)
        seen.add(verdict)
        if by_zlib is None:
            assert verdict != "ok", pos
        if verdict == "ok":                                               # (a flip in a filtered byte that keeps the Adler-32 does not exist)
            assert by_zlib is not None and px is not None
    assert zlib_rejects >= 20 and "ok" not in seen
    assert "adler" in seen and seen & {"bad-stream", "distance", "segment-size"}


def test_max_chunk_constant_is_the_librarys():
    from wu import _lib
    assert _lib.load().wu_png_dec_max_chunk_bytes() == D.MAX_CHUNK


# ---- (2) wu_png_dec_parse --------------------------------------------------------------------------------------------------------------------
def _c_parse(data, max_pixels=D.MAX_NATIVE_PIXELS):
    from wu import png
    info, idat = png.parse(data, max_pixels)
    return {"supported": bool(info.supported), "reason": info.reason_name, "h": info.height, "w": info.width,
            "idat": [(int(o), int(n)) for o, n in idat]}


def _same(data, max_pixels=D.MAX_NATIVE_PIXELS):
    """The C parser's verdict, after holding it against the restatement's."""
    got, want = _c_parse(data, max_pixels), D.parse(data, max_pixels)
    assert got["supported"] == want["supported"] and got["reason"] == want["reason"], (got, want["reason"])
    if want["supported"]:
        assert (got["h"], got["w"]) == (want["h"], want["w"]) and got["idat"] == want["idat"]
    return got


def test_parse_good_files():
    for variant in ("zlib6", "level0"):
        for name, (img, data) in D.zlib_fixtures(variant).items():
            got = _same(data)
            assert got["supported"] and (got["h"], got["w"]) == img.shape[:2], name
            assert len(got["idat"]) == -(-img.shape[0] * (1 + 3 * img.shape[1]) // D.SEGMENT)
            for off, ln in got["idat"]:
                assert data[off - 4:off] == b"IDAT" and struct.unpack(">I", data[off - 8:off - 4])[0] == ln
    for c in E.GRID[:4]:
        assert _same(E.encode(E.make_image(*c)))["supported"]


def test_parse_skips_ancillary_chunks():
    data = D.build(BIG)
    anc = D.with_ancillary(data)
    got = _same(anc)
    assert got["supported"] and len(got["idat"]) == 6
    assert [n for _, n in got["idat"]] == [n for _, n in _same(data)["idat"]]
    assert np.array_equal(_pillow(anc), BIG)
    assert D.decode(anc)[0] == "ok"


def test_parse_many_idat_chunks():
    """More IDAT chunks than the binding's first list holds: it calls again."""
    img = E.make_image(700, 1100, "gradient")
    data = D.build(img, level=1, filters=[1] * 700)
    got = _same(data)
    assert got["supported"] and len(got["idat"]) == -(-700 * 3301 // D.SEGMENT) > 64


def refusals():
    good = D.build(SMALL)
    big = D.build(BIG)
    cs = D.chunks(big)
    idat = [i for i, c in enumerate(cs) if c[1] == b"IDAT"]
    first = cs[idat[0]][0]
    second = cs[idat[1]][0]
    iend = cs[-1][0]
    out = [("not-png", b""), ("not-png", good[:7]), ("not-png", b"\xff\xd8\xff\xe0" + good[4:]), ("not-png", b"\x89PNG\r\n\x1a\r" + good[8:]),
           ("header", good[:8]), ("header", good[:32]), ("header", good[:29] + bytes([good[29] ^ 1]) + good[30:]),
           ("header", good[:8] + E.chunk(b"tEXt", b"a\0b") + good[8:]),
           ("header", good[:8] + E.chunk(b"IHDR", good[16:29] + b"\0") + good[33:]),
           ("header", _with_ihdr(good, w=0)), ("header", _with_ihdr(good, h=0)), ("header", _with_ihdr(good, comp=1)),
           ("header", _with_ihdr(good, flt=1)), ("header", _with_ihdr(good, lace=2)), ("header", _with_ihdr(good, w=0x80000000)),
           ("colour-type", _save(SMALL, "L")), ("colour-type", _save(SMALL, "RGBA")), ("colour-type", _save(SMALL, "P")),
           ("colour-type", _with_ihdr(good, colour=6, depth=16)),
           ("bit-depth", _with_ihdr(good, depth=16)), ("bit-depth", _with_ihdr(good, depth=4)),
           ("interlaced", _with_ihdr(good, lace=1)),
           ("too-large", _with_ihdr(good, w=10000, h=10000)), ("too-large", _with_ihdr(good, w=70000, h=1)),
           ("too-large", _with_ihdr(good, w=1, h=65536)),
           ("not-segmented", _save(BIG)), ("not-segmented", _with_ihdr(good, w=300, h=200)),
           ("not-segmented", big[:second] + big[cs[idat[2]][0]:]),                                   # one IDAT missing
           ("not-segmented", big[:second] + E.chunk(b"IDAT", b"") + big[second:]),                    # one too many
           ("not-segmented", D.rechunk(big, idat[0], b"\x78")),
           ("not-segmented", D.rechunk(big, idat[-1], b"\0\0\0")),
           ("not-segmented", D.rechunk(good, 1, b"\x78\x01\x03\0\0")),
           ("not-segmented", D.rechunk(big, idat[1], bytes(D.MAX_CHUNK + 1))),
           ("corrupt-chunk", good[:-12]),                                                            # no IEND
           ("corrupt-chunk", good[:33] + good[-12:]),                                                # no IDAT
           ("corrupt-chunk", big[:first] + E.chunk(b"PLTE", bytes(3)) + big[first:]),
           ("corrupt-chunk", big[:first] + E.chunk(b"NEWc", b"") + big[first:]),
           ("corrupt-chunk", big[:second] + E.chunk(b"tEXt", b"a\0b") + big[second:]),               # the IDAT run is interrupted
           ("corrupt-chunk", big[:iend] + b"\xff\xff\xff\xff" + big[iend + 4:]),
           ("corrupt-chunk", big[:second] + b"\xff\xff\xff\xff" + big[second + 4:]),
           ("corrupt-chunk", big[:second] + b"\x7f\xff\xff\xff" + big[second + 4:]),
           ("corrupt-chunk", D.rechunk(good, 1, b"\x79\x01" + good[43:])),                           # CM = 9
           ("corrupt-chunk", D.rechunk(good, 1, b"\x88\x1c" + good[43:])),                           # a 64 KiB window
           ("corrupt-chunk", D.rechunk(good, 1, b"\x78\x02" + good[43:])),                           # FCHECK
           ("corrupt-chunk", D.rechunk(good, 1, b"\x78\x20" + good[43:]))]                           # FDICT (FCHECK right: 0x7820 = 31 * 992)
    return out


def test_parse_every_refusal_reason():
    seen = set()
    for i, (reason, data) in enumerate(refusals()):
        got = _same(data)
        assert not got["supported"] and got["reason"] == reason, (i, reason, got["reason"])
        seen.add(reason)
    assert seen == set(D.REASONS.values()) - {"ok"}
    assert _same(D.build(BIG), max_pixels=200 * 300 - 1)["reason"] == "too-large"
    assert _same(D.build(BIG), max_pixels=200 * 300)["supported"]


def test_parse_truncations():
    """Every prefix of a small file, and of a six-segment file every chunk boundary and every cut inside a length field, a type or a
    CRC: never supported, never a read past the buffer (the restatement indexes a bytes object, the C parser a buffer of exactly
    that size), the same reason from both."""
    small = D.with_ancillary(D.build(SMALL))
    for n in range(len(small)):
        assert not _same(small[:n])["supported"], n
    assert _same(small)["supported"]
    big = D.with_ancillary(D.build(BIG))
    for at, _, ln in D.chunks(big):
        for cut in (at, at + 1, at + 3, at + 4, at + 7, at + 8, at + 8 + ln, at + 8 + ln + 3):
            got = _same(big[:cut])
            assert not got["supported"] and got["reason"] in ("header", "corrupt-chunk"), (at, cut, got)
    assert _same(big + b"trailing bytes")["supported"]


def test_parse_hostile_lengths():
    big = D.build(BIG)
    for at, _, _ in D.chunks(big)[1:]:
        for ln in (0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, len(big), len(big) - at - 11):
            assert _same(big[:at] + struct.pack(">I", ln) + big[at + 4:])["reason"] == "corrupt-chunk", (at, ln)
