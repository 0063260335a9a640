"""CPU: the glue of the PNG decoder's device stage (csrc/png_dec.hip, wu/png.py), as far as it runs without a GPU: the workspace layout
against its restatement, wu_png_dec_decode's refusal of every undersized buffer (the library loads without a device and validates
before it launches), the sizes wu.png hands over, and the fixtures of tests/_png_dec_cases.py themselves -- every one against the
restatement and Pillow, and the properties the GPU tests rely on (code lengths over 10 bits, all three repeat symbols in one header, the
degenerate distance codes, the block types), so that a change in zlib cannot silently empty those tests."""
import ctypes
import inspect

import numpy as np
import pytest

import _png_dec_cases as C
import _png_dec_ref as D


@pytest.fixture(scope="module")
def lib():
    from wu import _lib
    return _lib.load()


def test_workspace_bytes_matches_the_restated_layout(lib):
    shapes = [(1, 1, 1, 1), (1, 1, 1, 0), (3, 105, 104, 5), (3, 105, 104, 6), (3, 105, 104, 7), (2, 128, 85, 2), (64, 256, 256, 384),
              (7, 200, 300, 42), (1, 65535, 1, 6), (1, 1, 65535, 6), (4, 4096, 4096, 4 * 1537), (1, 65536, 1, 1), (1, 1, 65536, 1),
              (0, 4, 4, 0), (1, 0, 4, 0), (1, 4, 4, -1), (1, 20000, 20000, 1), (100, 8192, 8192, 100)]
    for n, h, w, s in shapes:
        assert lib.wu_png_dec_workspace_bytes(n, h, w, s) == C.workspace_bytes(n, h, w, s), (n, h, w, s)
    assert C.workspace_bytes(3, 105, 104, 6) == 3 * 65536 + 256 and C.workspace_bytes(3, 105, 104, 7) == 0
    assert C.workspace_bytes(1, 65536, 1, 1) == 0 and C.workspace_bytes(1, 20000, 20000, 1) == 0
    assert lib.wu_png_dec_desc_bytes() == 32 and lib.wu_png_dec_seg_bytes() == 16


def test_decode_refuses_every_undersized_buffer(lib):
    """Validation precedes the launches, so no device is needed: each buffer one byte short is refused by name; the addresses are
    never followed."""
    n, h, w, segs = 3, 105, 104, 5
    full = {"src": 12 * segs, "desc": 32 * n, "seg": 16 * segs, "ws": C.workspace_bytes(n, h, w, segs), "out": n * h * w * 3, "status": 4 * n}
    words = {"src": b"source", "desc": b"descriptor", "seg": b"segment table", "ws": b"workspace", "out": b"output", "status": b"status"}
    a = 0x10000                                           # aligned, non-null

    def call(sizes, n_=n, segs_=segs):
        return lib.wu_png_dec_decode(a, sizes["src"], a, sizes["desc"], a, sizes["seg"], segs_, a, sizes["ws"], a, sizes["out"], a,
                                     sizes["status"], n_, h, w, None)

    for key in full:
        rc = call(dict(full, **{key: full[key] - 1}))
        assert rc < 0 and words[key] in lib.wu_last_error(), (key, lib.wu_last_error())
    assert call(full, segs_=7) < 0 and b"bad shape" in lib.wu_last_error()           # more segments than three such images have
    assert call(full, n_=0) < 0
    assert lib.wu_png_dec_decode(None, 60, a, 96, a, 80, segs, a, full["ws"], a, full["out"], a, 12, n, h, w, None) < 0
    assert b"null" in lib.wu_last_error()
    assert lib.wu_png_dec_decode(a, 60, a, 96, a, 80, segs, a + 4, full["ws"], a, full["out"], a, 12, n, h, w, None) < 0
    assert b"aligned" in lib.wu_last_error()


def test_python_side_sizes_are_what_the_library_requires():
    from wu import png
    dec = png.GPUPngDecoder(threads=2)
    try:
        items = [C.CASES["dynamic_105x104"].file, C.non_native_file(), C.CASES["stored_6x2"].file]
        hb = dec.prepare(items)
        try:
            assert hb.sizes == [(105, 104), (12, 17), (6, 2)] and (hb.hmax, hb.wmax, hb.n_segments) == (105, 104, 3)
            assert dec.stats["fallback_reasons"] == {"colour-type": 1}
            s = dec.buffer_sizes(hb)
            assert s["workspace"] == C.workspace_bytes(3, 105, 104, 3) and s["out"] == 3 * 105 * 104 * 3 and s["status"] == 12
            assert s["desc"] == 96 and s["seg"] == 48 and s["source"] >= sum(len(i) for i in (items[0], items[2]))
            assert s["upload"] >= hb.off["seg"] + s["seg"] and hb.off["desc"] % 8 == 0 and hb.off["seg"] % 4 == 0
            desc = hb.staging.array[hb.off["desc"]:hb.off["desc"] + 96].view(png.DESC_DTYPE)
            seg = hb.staging.array[hb.off["seg"]:hb.off["seg"] + 48].view(png.SEG_DTYPE)
            assert desc["h"].tolist() == [105, 0, 6] and desc["nseg"].tolist() == [2, 0, 1] and desc["first_seg"].tolist() == [0, 0, 2]
            assert seg["image"].tolist() == [0, 0, 2] and seg["k"].tolist() == [0, 1, 0]
            for d, sg in ((desc[0], seg[0]), (desc[0], seg[1]), (desc[2], seg[2])):            # every body lies inside its file
                assert 8 <= sg["off"] and sg["off"] + sg["len"] + 4 <= d["file_bytes"] and d["src_off"] + d["file_bytes"] <= s["source"]
            if not __import__("torch").cuda.is_available():
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    dec.finish(hb)
        finally:
            hb.release()
    finally:
        dec.close()
    assert inspect.signature(png.decode_mixed).parameters["decoder"].default is None


def test_the_switches_are_off_by_default():
    from wu import data, fid
    assert inspect.signature(fid.statistics_of_path).parameters["gpu_decode_png"].default is False
    assert inspect.signature(fid.calculate_fid_given_paths).parameters["gpu_decode_png"].default is False
    assert inspect.signature(data.JpegBatchLoader.__init__).parameters["png_decode"].default is False


@pytest.mark.parametrize("group", C.GROUPS)
def test_fixtures_against_restatement_and_pillow(group):
    """Every fixture passes the parser; valid ones decode to Pillow's pixels, corrupt ones get the status the format's rules give."""
    assert C.names(group)
    for name in C.names(group):
        case = C.CASES[name]
        assert D.parse(case.file)["supported"], name
        verdict, px = C.expected(name)
        if case.want is None:
            assert verdict == "ok" and np.array_equal(px, C.pillow(case.file)), name
        else:
            assert verdict == case.want and px is None, (name, verdict)


def _kinds(name, keep_empty=False):
    return [b["type"] for b in C.file_blocks(C.CASES[name].file) if keep_empty or not b.get("empty")]


def test_fixtures_hold_the_block_types_their_names_promise():
    for hw in ("105x104", "128x85", "6x2"):
        assert set(_kinds(f"stored_{hw}", True)) == {0}
        assert set(_kinds(f"fixed_{hw}")) == {1}
    for name in ("dynamic_105x104", "dynamic_128x85", "dynamic_long_codes", "dynamic_matches", "dynamic_encoder_75x100"):
        assert 2 in _kinds(name), name
    assert set(_kinds("dynamic_128x85")) == {2} and set(_kinds("dynamic_long_codes")) == {2}
    mixed = C.file_blocks(C.CASES["mixed_blocks"].file)
    assert {b["type"] for b in mixed if not b.get("empty")} == {0, 1, 2} and sum(1 for b in mixed if b.get("empty")) == 2
    assert len(C.segments(C.CASES["dynamic_105x104"].file)) == 2                     # 32 865 filtered bytes: 32 768 + 97
    assert any(b.get("empty") for b in C.file_blocks(C.CASES["dynamic_105x104"].file))   # what Z_FULL_FLUSH leaves behind
    assert len(C.segments(C.CASES["dynamic_128x85"].file)) == 1 and 128 * (1 + 3 * 85) == C.SEGMENT


def test_fixtures_leave_the_fast_table_and_use_every_repeat_symbol():
    (long_codes,) = C.file_blocks(C.CASES["dynamic_long_codes"].file)
    assert max(long_codes["lit"]) > 10
    assert max(max(b["lit"]) for b in C.file_blocks(C.CASES["dynamic_105x104"].file) if b["lit"]) > 10
    (rep,) = C.file_blocks(C.CASES["dynamic_repeat_symbols"].file)
    assert {16, 17, 18} <= rep["cl_symbols"]
    (one,) = C.file_blocks(C.CASES["dynamic_one_distance_code"].file)
    assert one["dist"] == [1]
    (none,) = C.file_blocks(C.CASES["dynamic_no_distance_code"].file)
    assert none["dist"] == [0]
    (enc,) = C.file_blocks(C.CASES["dynamic_encoder_75x100"].file)
    assert enc["dist"] == [1]                                                       # the encoder's single, never used distance code


def test_match_fixture_holds_the_matches_it_promises():
    """Distances 1, 2, 3 with length 258, a distance not smaller than its length, a match from byte 0: read back from the stream."""
    (seg,) = C.segments(C.CASES["dynamic_matches"].file)
    br = D._Bits(seg)
    assert (br.take(1), br.take(2)) == (1, 2)
    lit_lens, dist_lens, _ = C.dynamic_header(br)
    lit, dist = D._Code(lit_lens, True), D._Code(dist_lens, True)
    at, found = 0, []
    while True:
        sym = lit.decode(br)
        if sym == 256:
            break
        if sym < 256:
            at += 1
            continue
        ln = D.LEN_BASE[sym - 257] + br.take(D.LEN_EXTRA[sym - 257])
        ds = dist.decode(br)
        found.append((ln, D.DIST_BASE[ds] + br.take(D.DIST_EXTRA[ds]), at))
        at += ln
    assert [(l, d) for l, d, _ in found[:3]] == [(258, 1), (258, 2), (258, 3)]
    assert any(d >= l for l, d, _ in found) and any(d == pos for _, d, pos in found)
