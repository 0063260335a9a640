"""GPU: the PNG decoder's device stage (csrc/png_dec.hip: one wave per segment inflates, one wave per image unfilters; wu/png.py).  PNG is
lossless, so every comparison is bit-exact.  The files come from tests/_png_dec_cases.py -- zlib per 32 KiB segment, a small deflate
writer for what zlib never emits -- and tests/test_png_dec_glue_cpu.py holds them against the restatement tests/_png_dec_ref.py and
Pillow on the CPU and asserts the properties relied on here (block types, code lengths over 10 bits, the repeat symbols, the degenerate
distance codes).  Expected pixels are the restatement's, which that test shows equal to Pillow's; a valid file must come back with
``stats["fallback"]`` unchanged, a corrupt one with the restatement's status, an all-zero slot and its neighbours unharmed."""
import zlib

import numpy as np
import pytest
import torch

import _png_dec_cases as C
import _png_dec_ref as D
import _png_enc_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dec():
    from wu.png import GPUPngDecoder
    d = GPUPngDecoder(DEV)
    yield d
    d.close()


def _check_batch(dec, names, what):
    """One batch of valid fixtures: pixels, sizes, zero padding, nothing through Pillow."""
    want = [C.expected(n)[1] for n in names]
    fb0, native0 = dec.stats["fallback"], dec.stats["native"]
    out, sizes, statuses = dec.decode_batch([C.CASES[n].file for n in names], return_status=True)
    got = out.cpu().numpy()
    assert statuses == ["ok"] * len(names), (what, dict(zip(names, statuses)))
    assert sizes == [w.shape[:2] for w in want], what
    assert got.shape == (len(names), max(h for h, _ in sizes), max(w for _, w in sizes), 3) and got.dtype == np.uint8
    assert dec.stats["fallback"] == fb0 and dec.stats["native"] == native0 + len(names), (what, dec.stats)
    for i, (name, img) in enumerate(zip(names, want)):
        h, w = img.shape[:2]
        bad = np.argwhere(got[i, :h, :w] != img)
        assert bad.size == 0, f"{what} {name} ({h} x {w}): {len(bad)} bytes differ, the first at (y, x, c) = {tuple(bad[0])}"
        assert not got[i, h:].any() and not got[i, :, w:].any(), f"{what} {name}: padding not zero"


def _group(dec, group):
    names = C.names(group)
    for n in names:                                       # each file alone in its batch
        _check_batch(dec, [n], group)
    _check_batch(dec, names, f"{group} (one batch)")      # and all of them together: mixed sizes, zero padding


def test_stored_blocks(dec):
    """level 0: 1 x 1, one row, one column, a row length that is no multiple of 4, two segments (32 768 + 97 bytes), exactly 32 768."""
    _group(dec, "stored")


def test_fixed_blocks(dec):
    """Z_FIXED on the same geometries."""
    _group(dec, "fixed")


def test_dynamic_blocks(dec):
    """zlib's dynamic blocks on the same geometries, the empty stored block of Z_FULL_FLUSH between the segments; codes of 11 to 15
    bits (behind the 10-bit table); 16, 17 and 18 in one header; a single distance code of length 1, used, and none at all; distance
    1, 2 and 3 with length 258, a distance larger than its length, a match from byte 0; the encoder's literal-only block."""
    _group(dec, "dynamic")


def _device_stage(dec, hb, fill=7):
    """The two launches alone on a prepared batch, into a poisoned output: (status codes, output as numpy)."""
    from wu import _lib
    from wu.layout import stream_ptr
    s = dec.buffer_sizes(hb)
    buf = hb.staging.tensor[:hb.used].to(DEV)
    ws = torch.full((s["workspace"],), 0xCC, dtype=torch.uint8, device=DEV)
    out = torch.full((hb.n, hb.hmax, hb.wmax, 3), fill, dtype=torch.uint8, device=DEV)
    status = torch.full((hb.n,), -1, dtype=torch.int32, device=DEV)
    base = buf.data_ptr()
    _lib.call("wu_png_dec_decode", base, s["source"], base + hb.off["desc"], s["desc"], base + hb.off["seg"], s["seg"], hb.n_segments,
              ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), status.data_ptr(), status.numel() * 4, hb.n, hb.hmax, hb.wmax, stream_ptr())
    return status.cpu().tolist(), out.cpu().numpy()


CORRUPT = C.names("corrupt")


@pytest.mark.parametrize("name", CORRUPT)
def test_corrupt_file_gets_its_status_and_a_zero_slot(dec, name):
    """Between two good files of other sizes: the restatement's status, every byte of the slot zero, the neighbours bit-exact."""
    codes = {v: k for k, v in D.STATUS.items()}
    case = C.CASES[name]
    assert C.expected(name)[0] == case.want
    a, b = "dynamic_long_codes", "fixed_105x104"
    hb = dec.prepare([C.CASES[a].file, case.file, C.CASES[b].file])
    try:
        status, got = _device_stage(dec, hb)
    finally:
        hb.release()
    assert status == [0, codes[case.want], 0], [D.STATUS.get(s, s) for s in status]
    assert not got[1].any()
    for i, n in ((0, a), (2, b)):
        img = C.expected(n)[1]
        h, w = img.shape[:2]
        assert np.array_equal(got[i, :h, :w], img) and not got[i, h:].any() and not got[i, :, w:].any(), n


def test_all_block_types_in_one_segment(dec):
    """Stored, fixed and dynamic blocks and two empty stored blocks in one segment."""
    _check_batch(dec, ["mixed_blocks"], "mixed blocks")


def test_all_filter_types_across_the_64_row_hand_over(dec):
    """Five filter types in one image; Paeth, Up and Average on rows 64 and 128, whose upper neighbour another 64-row group wrote."""
    _group(dec, "rest")


def test_mixed_batch_through_decode_mixed(dec):
    """Three sizes and a palette file Pillow decodes, through decode_mixed: input order kept, every slot's padding exactly zero."""
    from wu.png import decode_mixed
    names = ["filters_130x5", "dynamic_105x104", "stored_1x7"]
    palette = C.non_native_file()
    items = [C.CASES[names[0]].file, palette, C.CASES[names[1]].file, C.CASES[names[2]].file]
    want = [C.expected(names[0])[1], C.pillow(palette), C.expected(names[1])[1], C.expected(names[2])[1]]
    native0, reasons0 = dec.stats["native"], dec.stats["fallback_reasons"].get("colour-type", 0)
    out, sizes = decode_mixed(items, decoder=dec)
    got = out.cpu().numpy()
    assert sizes == [w.shape[:2] for w in want] and got.shape == (4, 130, 104, 3)
    assert dec.stats["native"] == native0 + 3 and dec.stats["fallback_reasons"]["colour-type"] == reasons0 + 1
    for i, img in enumerate(want):
        h, w = img.shape[:2]
        assert np.array_equal(got[i, :h, :w], img), i
        assert not got[i, h:].any() and not got[i, :, w:].any(), i
    out2, sizes2 = decode_mixed(items)                                      # a decoder of its own
    assert torch.equal(out, out2) and sizes2 == sizes


def test_device_rejection_goes_to_pillow(dec):
    """A valid PNG whose second segment reaches into the first (Z_SYNC_FLUSH): the device says `distance`, Pillow decodes it."""
    data, img = C.image_file(105, 104, flush=zlib.Z_SYNC_FLUSH)
    assert D.decode(data)[0] == "distance" and np.array_equal(C.pillow(data), img)
    before = dec.stats["fallback_reasons"].get("distance", 0)
    out, sizes, statuses = dec.decode_batch([C.CASES["stored_9x1"].file, data], return_status=True)
    assert statuses == ["ok", "distance"] and sizes == [(9, 1), (105, 104)]
    assert dec.stats["fallback_reasons"]["distance"] == before + 1
    got = out.cpu().numpy()
    assert np.array_equal(got[1], img) and np.array_equal(got[0, :9, :1], C.expected("stored_9x1")[1]) and not got[0, 9:].any() and not got[0, :, 1:].any()


def test_round_trip_through_the_encoder(dec):
    """GPUPngEncoder's files back through the decoder: bit-exact against the tensor that was encoded, nothing through Pillow."""
    from wu.png_enc import GPUPngEncoder
    enc = GPUPngEncoder(DEV)
    try:
        imgs = np.stack([E.make_image(105, 104, c, seed=3) for c in ("natural", "noise", "gradient_noise", "flat")])
        x = torch.from_numpy(imgs).to(DEV)
        files = enc.encode_batch(x)
    finally:
        enc.close()
    native0, fb0 = dec.stats["native"], dec.stats["fallback"]
    out, sizes = dec.decode_batch(files)
    assert torch.equal(out, x) and sizes == [(105, 104)] * 4
    assert dec.stats["native"] == native0 + 4 and dec.stats["fallback"] == fb0
