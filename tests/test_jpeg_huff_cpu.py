"""CPU: the host half of the device Huffman decoder (csrc/jpeg_huff.hip: wu_jpeg_scan_stage) against its Python restatement
(_jpeg_huff_ref.py), the restatement's walk against the host decoder (wu.jpeg.entropy_decode), and the argument checks of
wu_jpeg_huff_decode, which launch nothing.  The kernels themselves run in test_gpu_jpeg_huff.py (and, on the CPU under sanitizers, in
scratch/jpeg_huff_emu.cpp)."""
import ctypes
import os

import numpy as np
import pytest

import _jpeg_huff_ref as H
import _jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
SIZES = [(1, 1), (8, 8), (16, 16), (33, 17), (97, 131)]
SUBSEQ = [64, 128, 1024]
RESTART = ["restart_blocks.jpg", "restart_rows.jpg", "restart_grey.jpg"]


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def _same_stage(got, ref):
    assert bytes(got["scan"]) == ref["scan"]
    assert [tuple(int(v) for v in row) for row in got["segs"]] == ref["segs"]
    assert bytes(got["dht"]) == ref["dht"]
    assert np.array_equal(got["qtab"], ref["qtab"])
    assert got["n_subseq"] == ref["n_subseq"]
    # the layout the kernels lean on: 16-byte multiples inside the promised bound, 8 zero bytes behind the last subsequence, every
    # segment on a subsequence boundary with at least one subsequence
    assert len(got["scan"]) % 16 == 0 and len(got["scan"]) <= got["bound"]


@pytest.mark.parametrize("S", SUBSEQ + [4096])
def test_scan_stage_equals_the_restatement(S):
    from wu import jpeg
    cases = R.grid() + [(n, _golden(n)) for n in RESTART]
    for name, data in cases:
        got = jpeg.scan_stage(data, S)
        ref = H.scan_stage(data, got["info"], S)
        _same_stage(got, ref)
        sub = S // 8
        assert len(got["scan"]) >= got["n_subseq"] * sub + 8 and not got["scan"][got["n_subseq"] * sub:].any(), name
        first = got["segs"][:, 0]
        assert first[0] == 0 and (np.diff(first) >= 1).all() and first[-1] < got["n_subseq"], name
        assert (got["segs"][:, 1] <= np.diff(np.append(first, got["n_subseq"])) * S).all(), name
        _, qt, _ = jpeg.entropy_decode(data)
        assert np.array_equal(got["qtab"], qt), name
    # restart intervals were among them: the three fixtures, and q30_444_rst1 at the 8 sizes of more than one 8x8 MCU
    assert sum(len(jpeg.scan_stage(d, S)["segs"]) > 1 for _, d in cases) >= 11


def test_scan_stage_removes_stuffing_and_splits_at_restart_markers():
    from wu import jpeg
    data = _golden("restart_blocks.jpg")
    info = jpeg.parse(data)
    assert info.restart_interval > 0
    st = jpeg.scan_stage(data, 64)
    raw = data[info.scan_offset:]
    body = b"".join(bytes(st["scan"][f * 8:f * 8 + bits // 8]) for f, bits, _, _ in st["segs"])
    # the same bytes the file holds between SOS and EOI, without the stuffed zeros and the RSTn markers
    plain, i = bytearray(), 0
    while i < len(raw):
        if raw[i] == 0xFF and raw[i + 1] == 0:
            plain.append(0xFF)
            i += 2
        elif raw[i] == 0xFF and 0xD0 <= raw[i + 1] <= 0xD7:
            i += 2
        elif raw[i] == 0xFF:
            break
        else:
            plain.append(raw[i])
            i += 1
    assert body == bytes(plain)
    mcus = info.mcus_x * info.mcus_y
    assert st["segs"][:, 3].sum() == mcus and list(st["segs"][:, 2]) == list(range(0, mcus, info.restart_interval))


def test_scan_stage_refusals_and_truncated_file():
    from wu import _lib, jpeg
    lib = _lib.load()
    data = bytearray(_golden("restart_blocks.jpg"))
    info = jpeg.parse(bytes(data))
    marks = [i for i in range(info.scan_offset, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(marks) >= 2
    data[marks[0] + 1], data[marks[1] + 1] = data[marks[1] + 1], data[marks[0] + 1]          # RST1 in front of RST0
    with pytest.raises(jpeg.JpegError, match="restart marker"):
        jpeg.scan_stage(bytes(data), 1024)
    with pytest.raises(jpeg.JpegError):                                # the host decoder refuses the same file
        jpeg.entropy_decode(bytes(data))
    with pytest.raises(H.StageError) as e:
        H.scan_stage(bytes(data), info, 1024)
    assert e.value.code == -3

    good = _golden("restart_rows.jpg")
    info = jpeg.parse(good)
    bound = lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), len(good), 1024)
    nseg = lib.wu_jpeg_scan_segments(ctypes.byref(info))
    assert bound > 0 and bound % 16 == 0 and nseg == H.n_segments(info) > 1
    scan, segs = np.zeros(bound, np.uint8), np.zeros((nseg, 4), np.int32)
    dht, qtab, res = np.zeros(jpeg.DHT_BYTES, np.uint8), np.zeros(192, np.uint16), jpeg.JpegScan()

    def stage(scan_cap, seg_cap, S=1024, info=info):
        return lib.wu_jpeg_scan_stage(good, len(good), ctypes.byref(info), S, scan.ctypes.data, scan_cap, segs.ctypes.data, seg_cap,
                                      dht.ctypes.data, qtab.ctypes.data, ctypes.byref(res))
    assert stage(bound, segs.nbytes) == 0 and res.n_segments == nseg and 0 < res.scan_bytes <= bound
    assert stage(bound - 16, segs.nbytes) < 0 and b"capacity" in lib.wu_last_error()
    assert stage(bound, segs.nbytes - 16) < 0 and b"capacity" in lib.wu_last_error()
    assert stage(bound, segs.nbytes, S=48) < 0 and b"subseq_bits" in lib.wu_last_error()
    assert stage(bound, segs.nbytes, S=8192) < 0 and b"subseq_bits" in lib.wu_last_error()
    assert lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), len(good), 48) == 0
    unsupported = jpeg.parse(_golden("progressive.jpg"))
    assert lib.wu_jpeg_scan_stage_bytes(ctypes.byref(unsupported), 1000, 1024) == 0 and lib.wu_jpeg_scan_segments(ctypes.byref(unsupported)) == 0
    assert stage(bound, segs.nbytes, info=unsupported) < 0 and b"supported" in lib.wu_last_error()
    with pytest.raises(jpeg.JpegUnsupported):
        jpeg.scan_stage(_golden("progressive.jpg"))

    cut = _golden("truncated.jpg")                                      # stages without error: only decoding finds the end
    st = jpeg.scan_stage(cut, 128)
    _same_stage(st, H.scan_stage(cut, st["info"], 128))
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_decode(cut)
    _, _, status, _ = H.decode(cut, st["info"], 128)
    assert status & H.SHORT


def test_scan_stage_bound_keeps_bit_positions_in_32_bits():
    from wu import _lib, jpeg
    lib = _lib.load()
    info = jpeg.parse(R.grid([(16, 16)], R.VARIANTS[:1])[0][1])
    assert lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), (1 << 28) - 4096, 1024) > 0
    assert lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), (1 << 28) + info.scan_offset, 1024) == 0       # reported, never wrapped


@pytest.fixture(scope="module")
def host_coefficients():
    from wu import jpeg
    out = {}
    for name, data in R.grid(SIZES):
        planes, qt, info = jpeg.entropy_decode(data)
        out[name] = (data, info, np.concatenate([p.reshape(-1, 64) for p in planes]), qt)
    return out


@pytest.mark.parametrize("S", SUBSEQ)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restated_walk_equals_the_host_decoder(host_coefficients, size, S):
    """Rounds, carry, count, write and DC scan of the restatement give wu.jpeg.entropy_decode's blocks for every variant, and the
    walk's exit states are the sequential decoder's."""
    seen = 0
    for name, (data, info, want, qt) in host_coefficients.items():
        if not name.startswith(f"{size[0]}x{size[1]}_"):
            continue
        coef, qtab, status, w = H.decode(data, info, S)
        assert status == 0, name
        assert np.array_equal(coef, want), f"{name}: {np.count_nonzero(coef != want)} coefficients differ"
        assert np.array_equal(qtab, qt), name
        assert w.exits == H.sequential_exits(w), name
        if name == "97x131_q100_444" and S == 64:
            # the worst case: more than one chunk with carried states, and a chunk in which thread 0's exact state is the last to
            # arrive, after all 255 rounds
            assert w.nsub > 20 * H.CHUNK and max(w.rounds) == H.CHUNK - 1
        seen += 1
    assert seen == len(R.VARIANTS)


def test_restatement_reports_the_magnitude_bound():
    from wu import jpeg
    noise = (np.random.default_rng(7).integers(0, 2, (64, 64, 1)) * 255).astype(np.uint8).repeat(3, 2)
    data = R.encode(noise, dict(quality=100, subsampling=0))
    with pytest.raises(jpeg.JpegUnsupported, match="magnitude"):
        jpeg.entropy_decode(data)
    assert H.decode(data, jpeg.parse(data), 1024)[2] == H.MAGNITUDE


def test_huff_decode_argument_errors_without_a_gpu():
    """Validated on the host before anything is launched."""
    from wu import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    p = (p + 15) & ~15
    assert lib.wu_jpeg_huff_desc_bytes() == 64
    assert lib.wu_jpeg_huff_decode(None, p, p, p, p, p, p, 1, 1024, None) < 0 and b"null" in lib.wu_last_error()
    assert lib.wu_jpeg_huff_decode(p, p, p, p, p, None, p, 1, 1024, None) < 0 and b"null" in lib.wu_last_error()
    assert lib.wu_jpeg_huff_decode(p, p, p, p, p, p, None, 1, 1024, None) < 0 and b"null" in lib.wu_last_error()
    for bad in (48, 8192, 0, 100):
        assert lib.wu_jpeg_huff_decode(p, p, p, p, p, p, p, 1, bad, None) < 0 and b"subseq_bits" in lib.wu_last_error()
    assert lib.wu_jpeg_huff_decode(p, p, p, p, p, p, p, 0, 1024, None) < 0 and b"batch size" in lib.wu_last_error()
    assert lib.wu_jpeg_huff_decode(p, p, p, p, p, p + 2, p, 1, 1024, None) < 0 and b"misaligned" in lib.wu_last_error()


def test_decoder_options_are_checked_without_a_gpu():
    from wu.jpeg import GPUJpegDecoder
    with pytest.raises(ValueError, match="entropy"):
        GPUJpegDecoder(entropy="gpu")
    with pytest.raises(ValueError, match="subseq_bits"):
        GPUJpegDecoder(entropy="device", subseq_bits=48)
    dec = GPUJpegDecoder("cpu", threads=2, entropy="device", subseq_bits=128)
    cases = R.grid([(33, 17)], R.VARIANTS[:2])
    hb = dec.prepare([d for _, d in cases] + [_golden("progressive.jpg")])           # staging needs no GPU
    assert hb.entropy == "device" and hb.last_status == ["ok", "ok", "progressive"] and dec.stats["fallback"] == 1
    assert list(hb.off) == ["scan", "seg", "dht", "qtab", "hdesc", "desc", "tile"] and "coef" not in hb.off
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.finish(hb)
    hb.release()
    dec.close()
    assert GPUJpegDecoder("cpu").entropy == "host"
