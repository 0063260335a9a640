"""CPU: the extended coverage of the JPEG host stage (csrc/jpeg_host.h: wu_jpeg_parse_ex, the progressive scans of
wu_jpeg_entropy_decode; wu.jpeg ``coverage="extended"``) and the h1v2 chroma rule of 4:4:0 files through its numpy restatement
(tests/_jpeg_prog_ref.py).  Oracles: the BASELINE TWIN of a progressive file (same Pillow arguments without ``progressive``: the same
quantised coefficients) and Pillow's own decode.  Tolerance everywhere: exact equality.

The sanitizer run of the same host code is a stand-alone program (scratch/jpeg_prog_asan.cpp; command and result in DESIGN.md section 6b),
run by hand on a CPU: a sanitizer runtime must be the first library of its process, which a test cannot promise everywhere."""
import os

import numpy as np
import pytest

import _jpeg_prog_ref as P
import _jpeg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg")


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def _planes_equal(a, b):
    return len(a[0]) == len(b[0]) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


# ---- 1. defaults -------------------------------------------------------------------------------------------------------------------
def test_defaults_still_refuse():
    from wu import jpeg
    prog = P.twins((33, 17), 2)[0][1]
    for data in (prog, _golden("progressive.jpg")):
        for info in (jpeg.parse(data), jpeg.parse(data, coverage="baseline")):
            assert info.supported == 0 and info.reason_name == "progressive"
        with pytest.raises(jpeg.JpegUnsupported) as e:
            jpeg.entropy_decode(data)
        assert e.value.reason == "progressive"
    for data in (P.make_440(16), P.make_440(17, progressive=False), _golden("s440.jpg")):
        info = jpeg.parse(data)
        assert info.supported == 0 and info.reason_name == "sampling"
    assert jpeg.parse(P.make_440(16, progressive=True)).reason_name == "progressive"        # the frame kind is met first
    with pytest.raises(ValueError, match="coverage"):
        jpeg.parse(prog, coverage="everything")
    with pytest.raises(ValueError, match="coverage"):
        jpeg.entropy_decode(prog, coverage="")
    assert jpeg.REASONS[12] == "progressive-incomplete" and jpeg.MODE_H1V2 == 4


def test_parse_extended_reports_the_frame_kind_in_the_same_struct():
    import ctypes
    from wu import _lib, jpeg
    assert _lib.load().wu_jpeg_info_bytes() == ctypes.sizeof(jpeg.JpegInfo) == 192          # as before: the frame kind took the spare int
    img = R.synth(33, 17, 4)
    for kw, sampling in ((dict(quality=75), [(2, 2), (1, 1), (1, 1)]), (dict(quality=85, subsampling=1), [(2, 1), (1, 1), (1, 1)]), ("grey", [(1, 1)])):
        prog, base = P.encode(img, kw, True), P.encode(img, kw, False)
        ip, ib = jpeg.parse(prog, coverage="extended"), jpeg.parse(base, coverage="extended")
        assert ip.supported == 1 and ip.progressive and ip.reserved == jpeg.FRAME_PROGRESSIVE and ip.sampling == sampling
        assert ib.supported == 1 and not ib.progressive and ib.reserved == jpeg.FRAME_SEQUENTIAL
        for f in ("height", "width", "ncomp", "mode", "mcus_x", "mcus_y", "total_blocks", "coef_bytes"):
            assert getattr(ip, f) == getattr(ib, f), f
        sos = P.sos_offsets(prog)[0]
        assert ip.scan_offset == sos + 2 + ((prog[sos + 2] << 8) | prog[sos + 3])            # the first scan's data, as for a baseline file
        plain = jpeg.parse(base)
        assert bytes(plain) == bytes(ib)                                                      # the flags change nothing for a baseline file
    i440 = jpeg.parse(P.make_440(17), coverage="extended")
    assert i440.supported == 1 and i440.mode == jpeg.MODE_H1V2 and i440.sampling == [(1, 2), (1, 1), (1, 1)]
    assert (i440.mcus_x, i440.mcus_y, i440.blocks_w[0], i440.blocks_h[0], i440.blocks_w[1], i440.blocks_h[1]) == (3, 2, 3, 4, 3, 2)
    # what the flags do not add stays refused
    assert jpeg.parse(_golden("cmyk.jpg"), coverage="extended").reason_name == "colorspace"
    base = R.encode(R.synth(40, 56, 3), dict(quality=75))
    at = base.index(b"\xff\xc0")
    assert jpeg.parse(base[:at + 11] + b"\x41" + base[at + 12:], coverage="extended").reason_name == "sampling"       # 4:1:1
    prog = P.encode(R.synth(40, 56, 3), dict(quality=75), True)
    at = prog.index(b"\xff\xc2")
    assert jpeg.parse(prog[:at + 4] + b"\x0c" + prog[at + 5:], coverage="extended").reason_name == "precision"        # 12-bit progressive


# ---- 2. progressive coefficients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(enumerate(R.SMALL_SIZES)), ids=lambda s: f"{s[1][0]}x{s[1][1]}")
def test_progressive_scans_equal_the_baseline_twin_and_pillow(size):
    """Every case decodes natively: planes and tables equal the twin's, and the numpy reconstruction equals Pillow's decode of the
    PROGRESSIVE bytes."""
    from wu import jpeg
    cases = P.twins(size[1], size[0])
    assert len(cases) == len(P.PROG_VARIANTS) == 10
    for name, prog, base in cases:
        info = jpeg.parse(prog, coverage="extended")
        assert info.supported == 1 and info.progressive, f"{name}: {info.reason_name}"
        assert len(P.sos_offsets(prog)) == (6 if "grey" in name else 10), name                # libjpeg's standard script
        if "rst" in name:
            assert info.restart_interval > 0
        got, want = jpeg.entropy_decode(prog, coverage="extended"), jpeg.entropy_decode(base)
        assert _planes_equal(got, want), name
        assert got[2].max_block_l1 == want[2].max_block_l1, name
        rgb = R.reconstruct(got)
        ref = R.pillow_rgb(prog)
        assert rgb.shape == ref.shape and np.array_equal(rgb, ref), f"{name}: {np.count_nonzero(rgb != ref)} bytes differ"


def test_golden_progressive_file():
    from wu import jpeg
    data = _golden("progressive.jpg")
    got = R.reconstruct(jpeg.entropy_decode(data, coverage="extended"))
    assert np.array_equal(got, R.pillow_rgb(data))
    with np.load(os.path.join(GOLDEN, "expected.npz")) as exp:
        assert np.array_equal(got, exp["progressive.jpg"])


def test_a_one_component_scan_walks_the_components_own_grid():
    """4:2:0 at 17 x 33 and 33 x 17: the luma grid (3 x 5 blocks) is smaller than the MCU-padded plane (4 x 6), which only the
    interleaved DC scans fill."""
    from wu import jpeg
    for (h, w) in ((17, 33), (33, 17)):
        img = R.synth(h, w, 5)
        prog, base = P.encode(img, dict(quality=90), True), P.encode(img, dict(quality=90), False)
        got, want = jpeg.entropy_decode(prog, coverage="extended"), jpeg.entropy_decode(base)
        assert got[0][0].shape[:2] == (-(-h // 16) * 2, -(-w // 16) * 2) != (-(-h // 8), -(-w // 8))
        assert _planes_equal(got, want)


# ---- 3. 4:4:0 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
def test_440_restatement_equals_pillow(progressive):
    from wu import jpeg
    for side in P.SQUARE_440:
        data = P.make_440(side, seed=side, progressive=progressive)
        dec = jpeg.entropy_decode(data, coverage="extended")
        assert dec[2].mode == jpeg.MODE_H1V2 and dec[2].progressive == progressive
        got, want = P.reconstruct(dec), R.pillow_rgb(data)
        assert got.shape == want.shape == (side, side, 3) and np.array_equal(got, want), f"{side}: {np.count_nonzero(got != want)} bytes differ"


def test_golden_440_file():
    from wu import jpeg
    data = _golden("s440.jpg")
    got = P.reconstruct(jpeg.entropy_decode(data, coverage="extended"))
    assert np.array_equal(got, R.pillow_rgb(data))
    with np.load(os.path.join(GOLDEN, "expected.npz")) as exp:
        assert np.array_equal(got, exp["s440.jpg"])


# ---- 4. / 5. incomplete and truncated files -------------------------------------------------------------------------------------------
def test_incomplete_file_is_refused_and_prepare_reports_it():
    from wu import jpeg
    prog = P.twins((64, 48), 1)[0][1]
    n_scans = len(P.sos_offsets(prog))
    for keep in range(1, n_scans):
        cut = P.make_incomplete(prog, keep)
        assert jpeg.parse(cut, coverage="extended").supported == 1
        with pytest.raises(jpeg.JpegUnsupported) as e:
            jpeg.entropy_decode(cut, coverage="extended")
        assert e.value.reason == "progressive-incomplete", keep
        R.pillow_rgb(cut)                                                                     # a valid file: Pillow reads it
    dec = jpeg.GPUJpegDecoder(threads=2, coverage="extended")
    hb = dec.prepare([prog, P.make_incomplete(prog, 4), P.make_incomplete(prog, n_scans - 1)])
    assert hb.last_status == ["ok", "progressive-incomplete", "progressive-incomplete"]
    assert dec.stats == {"native": 1, "fallback": 2, "fallback_reasons": {"progressive-incomplete": 2}}
    assert [s for s, _ in hb.fallbacks] == [1, 2] and np.array_equal(hb.fallbacks[0][1], R.pillow_rgb(P.make_incomplete(prog, 4)))
    hb.release()
    dec.close()


def test_truncated_file_raises():
    from wu import jpeg
    prog = P.twins((97, 131), 0)[0][1]
    sos = P.sos_offsets(prog)
    cuts = [sos[0] + 40, (sos[2] + sos[3]) // 2, (sos[5] + sos[6]) // 2, len(prog) - 3, len(prog) - 2]      # inside scans; the last: EOI gone
    for cut in cuts:
        with pytest.raises(jpeg.JpegError):
            jpeg.entropy_decode(prog[:cut], coverage="extended")
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_decode(prog[:sos[4]], coverage="extended")                               # at an SOS boundary, without EOI


def test_illegal_scan_scripts():
    """Scan headers edited in place: what libjpeg raises an error for is a JpegError, what it only warns about is refused."""
    from wu import jpeg
    prog = bytearray(P.twins((33, 17), 3)[0][1])
    sos = P.sos_offsets(bytes(prog))

    def edited(scan, field, value):
        out = bytearray(prog)
        ns = out[sos[scan] + 4]
        out[sos[scan] + 5 + 2 * ns + field] = value
        return bytes(out)

    ns1 = prog[sos[1] + 4]
    assert ns1 == 1 and prog[sos[1] + 5 + 2 * ns1] == 1                                       # scan 1 of the script: Y, Ss = 1, Se = 5, Al = 2
    for data in (edited(1, 0, 9), edited(1, 1, 64), edited(0, 1, 5), edited(0, 2, 0x31), edited(1, 2, 0x0e)):   # Ss > Se, Se > 63, DC with AC, Al != Ah - 1, Al > 13
        with pytest.raises(jpeg.JpegError):
            jpeg.entropy_decode(data, coverage="extended")
    for data in (edited(1, 2, 0x21),):                                                        # a refinement (Ah = 2) of coefficients never sent
        with pytest.raises(jpeg.JpegUnsupported) as e:
            jpeg.entropy_decode(data, coverage="extended")
        assert e.value.reason == "progressive-incomplete"
    # an AC scan in front of its component's DC scan: drop the first scan
    no_dc = bytes(prog[:sos[0]]) + bytes(prog[sos[1]:])
    with pytest.raises(jpeg.JpegUnsupported) as e:
        jpeg.entropy_decode(no_dc, coverage="extended")
    assert e.value.reason == "progressive-incomplete"


# ---- 6. corrupt bytes ----------------------------------------------------------------------------------------------------------------
def test_flipped_bytes_never_crash():
    from wu import jpeg
    rng = np.random.default_rng(0)
    for prog in (P.twins((64, 48), 1, P.PROG_VARIANTS[:1])[0][1], P.twins((40, 3), 8, [P.PROG_VARIANTS[9]])[0][1],      # optimize: a DHT in front of every scan
                 P.make_440(33, progressive=True)):
        sos = P.sos_offsets(prog)
        dht_between = [i for i in range(sos[0], len(prog) - 1) if prog[i] == 0xFF and prog[i + 1] == 0xC4]
        where = list(range(sos[0], len(prog), 7))
        for at in dht_between:
            where += list(range(at, at + 40))
        outcomes = set()
        for at in where:
            bad = bytearray(prog)
            bad[at] = int(rng.integers(0, 256))
            try:
                planes, qt, info = jpeg.entropy_decode(bytes(bad), coverage="extended")
                assert sum(p.size for p in planes) == info.total_blocks * 64
                outcomes.add("planes")
            except jpeg.JpegError:
                outcomes.add("error")
            except jpeg.JpegUnsupported:
                outcomes.add("refused")
        assert {"planes", "error"} <= outcomes
    assert any(len(d) for d in [dht_between])                                                  # the last file had tables between its scans


# ---- 7. the decoder object -------------------------------------------------------------------------------------------------------------
def test_decoder_counts_extended_files_as_native():
    from wu import jpeg
    prog, base = P.twins((18, 34), 6)[0][1:]
    items = [base, prog, P.make_440(16), P.make_440(17, progressive=True), os.path.join(GOLDEN, "progressive.jpg"), os.path.join(GOLDEN, "s440.jpg"),
             os.path.join(GOLDEN, "cmyk.jpg")]
    dec = jpeg.GPUJpegDecoder(threads=2, coverage="extended")
    assert dec.coverage == "extended" and dec.entropy == "host"
    hb = dec.prepare(items)
    assert dec.stats == {"native": 6, "fallback": 1, "fallback_reasons": {"colorspace": 1}}
    assert hb.last_status == ["ok"] * 6 + ["colorspace"]
    desc = hb.staging.array[hb.off["desc"]:hb.off["desc"] + hb.n * 64].view(np.int32).reshape(hb.n, 16)
    assert list(desc[:, 3]) == [jpeg.MODE_H2V2, jpeg.MODE_H2V2, jpeg.MODE_H1V2, jpeg.MODE_H1V2, jpeg.MODE_H2V2, jpeg.MODE_H1V2, 0]
    # the staged coefficients of the progressive file are the twin's
    nb = int(desc[0, 9])
    coef = hb.staging.array[hb.off["coef"]:hb.off["qtab"]].view(np.int16).reshape(-1, 64)
    assert desc[1, 9] == nb and np.array_equal(coef[desc[0, 0]:desc[0, 0] + nb], coef[desc[1, 0]:desc[1, 0] + nb])
    hb.release()
    dec.close()
    # the default decoder on the same items: as before
    dec = jpeg.GPUJpegDecoder(threads=2)
    assert dec.coverage == "baseline"
    hb = dec.prepare(items)
    assert dec.stats == {"native": 1, "fallback": 6, "fallback_reasons": {"progressive": 3, "sampling": 2, "colorspace": 1}}
    hb.release()
    dec.close()


def test_decoder_arguments():
    from wu import files, jpeg
    from wu.data import JpegBatchLoader
    with pytest.raises(ValueError, match="entropy='host'"):
        jpeg.GPUJpegDecoder(coverage="extended", entropy="device")
    with pytest.raises(ValueError, match="coverage"):
        jpeg.GPUJpegDecoder(coverage="progressive")
    with files.pass_decoder(gpu_extended=True) as dec:
        assert isinstance(dec, jpeg.GPUJpegDecoder) and dec.coverage == "extended" and dec.entropy == "host"
    with files.pass_decoder(gpu_decode=True) as dec:
        assert dec.coverage == "baseline"
    with pytest.raises(ValueError):
        with files.pass_decoder(gpu_entropy=True, gpu_extended=True):
            pass
    ld = JpegBatchLoader([os.path.join(GOLDEN, "progressive.jpg")], jpeg_coverage="extended")
    assert ld.decoder.coverage == "extended"
    ld.decoder.close()
    ld = JpegBatchLoader([os.path.join(GOLDEN, "progressive.jpg")])
    assert ld.decoder.coverage == "baseline"
    ld.decoder.close()


def test_device_staging_refuses_extended_infos():
    """The C ABI of the device Huffman path on an info only wu_jpeg_parse_ex hands out: no staging bound, no segments."""
    import ctypes
    from wu import _lib, jpeg
    lib = _lib.load()
    for data in (P.twins((16, 16), 0)[0][1], P.make_440(16)):
        info = jpeg.parse(data, coverage="extended")
        assert info.supported == 1
        assert lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), len(data), 1024) == 0 and lib.wu_jpeg_scan_segments(ctypes.byref(info)) == 0
