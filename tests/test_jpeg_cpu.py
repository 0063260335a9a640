"""CPU: the host half of the JPEG decoder (csrc/jpeg.hip: wu_jpeg_parse, wu_jpeg_entropy_decode; wu/jpeg.py) and the batch loader
(wu/data.py).  The arithmetic the device kernels implement is pinned here through its numpy restatement (tests/_jpeg_ref.py):
Huffman stage + restatement == Pillow, byte for byte.  Tolerance everywhere: exact equality."""
import gc
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


# ---- 1. parse -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,sampling", [("q75_420", dict(quality=75), [(2, 2), (1, 1), (1, 1)]),
                                              ("q90_444", dict(quality=90, subsampling=0), [(1, 1), (1, 1), (1, 1)]),
                                              ("q85_422", dict(quality=85, subsampling=1), [(2, 1), (1, 1), (1, 1)]),
                                              ("opt", dict(quality=75, optimize=True), [(2, 2), (1, 1), (1, 1)]),
                                              ("grey", "grey", [(1, 1)])])
def test_parse_supported(name, kw, sampling):
    from wu import jpeg
    for (h, w) in [(97, 131), (1, 1), (375, 500)]:
        info = jpeg.parse(R.encode(R.synth(h, w, 1), kw))
        assert info.supported == 1 and info.reason_name == "ok"
        assert (info.height, info.width) == (h, w) and info.sampling == sampling and info.restart_interval == 0
        hmax, vmax = sampling[0]
        assert (info.mcus_x, info.mcus_y) == (-(-w // (8 * hmax)), -(-h // (8 * vmax)))
        assert info.total_blocks == sum(info.mcus_x * sh * info.mcus_y * sv for sh, sv in sampling)
        assert info.coef_bytes == info.total_blocks * 128


def test_parse_golden_files():
    from wu import jpeg
    want = {"baseline_420.jpg": (1, "ok", 0), "restart_blocks.jpg": (1, "ok", 2), "restart_rows.jpg": (1, "ok", 5), "restart_grey.jpg": (1, "ok", 1),
            "progressive.jpg": (0, "progressive", 0), "cmyk.jpg": (0, "colorspace", 0), "s440.jpg": (0, "sampling", 0),
            "rgb.png": (0, "not-jpeg", 0), "grey.png": (0, "not-jpeg", 0), "truncated.jpg": (1, "ok", 0)}     # its HEADER is whole
    for name, (sup, reason, ri) in want.items():
        info = jpeg.parse(os.path.join(GOLDEN, name))
        assert (info.supported, info.reason_name, info.restart_interval) == (sup, reason, ri), name
    assert jpeg.parse(os.path.join(GOLDEN, "restart_rows.jpg")).sampling == [(2, 1), (1, 1), (1, 1)]
    assert jpeg.parse(os.path.join(GOLDEN, "s440.jpg")).sampling == [(1, 2), (1, 1), (1, 1)]


def _patched(data, marker, offset, value):
    at = data.index(marker)
    return data[:at + offset] + bytes([value]) + data[at + offset + 1:]


def test_parse_reports_what_it_does_not_decode():
    """Header variants no encoder at hand writes, made by editing a baseline file's header: reported, never guessed at."""
    from wu import jpeg
    base = R.encode(R.synth(40, 56, 3), dict(quality=75))
    assert jpeg.parse(_patched(base, b"\xff\xc0", 4, 12)).reason_name == "precision"                  # 12-bit samples
    assert jpeg.parse(_patched(base, b"\xff\xc0", 1, 0xC9)).reason_name == "arithmetic"               # SOF9
    assert jpeg.parse(_patched(base, b"\xff\xc0", 1, 0xC3)).reason_name == "lossless"                 # SOF3
    assert jpeg.parse(_patched(base, b"\xff\xc0", 11, 0x41)).reason_name == "sampling"                # luma 4x1 (4:1:1)
    assert jpeg.parse(_patched(base, b"\xff\xc0", 14, 0x22)).reason_name == "sampling"                # sub-sampled chroma factors 2x2
    assert jpeg.parse(_patched(base, b"\xff\xda", 4, 1)).reason_name in ("multiscan", "corrupt-header")   # a scan of one component
    at = base.index(b"\xff\xdb")
    assert jpeg.parse(base[:at + 4] + bytes([0x10 | base[at + 4]]) + base[at + 5:]).reason_name == "corrupt-header"   # 16-bit table, 8-bit length
    for cut in (3, 20, at + 30, base.index(b"\xff\xc4") + 10, base.index(b"\xff\xda") + 3):
        info = jpeg.parse(base[:cut])
        assert info.supported == 0 and info.reason_name in ("corrupt-header", "not-jpeg"), cut
    assert jpeg.parse(b"").reason_name == "not-jpeg" and jpeg.parse(b"GIF89a" + bytes(40)).reason_name == "not-jpeg"
    # an RGB-tagged file: no JFIF marker, component ids 'R', 'G', 'B'
    app0 = base.index(b"\xff\xe0")
    ln = (base[app0 + 2] << 8) | base[app0 + 3]
    rgb = base[:app0] + base[app0 + 2 + ln:]
    assert jpeg.parse(rgb).supported == 1                                                              # ids 1, 2, 3 without JFIF: YCbCr
    sof = rgb.index(b"\xff\xc0")
    sos = rgb.index(b"\xff\xda")
    rgb = bytearray(rgb)
    for c, ch in enumerate(b"RGB"):
        rgb[sof + 10 + 3 * c] = ch
        rgb[sos + 5 + 2 * c] = ch
    assert jpeg.parse(bytes(rgb)).reason_name == "colorspace"


# ---- 2. host stage + arithmetic pin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.SMALL_SIZES + R.LARGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entropy_decode_plus_restatement_equals_pillow(size):
    """Every case of the grid decodes natively (no JpegUnsupported) and reconstructs to Pillow's bytes."""
    from wu import jpeg
    cases = R.grid([size])
    assert len(cases) == len(R.VARIANTS) >= 13
    for name, data in cases:
        info = jpeg.parse(data)
        assert info.supported == 1, f"{name}: {info.reason_name}"
        if "rst" in name:
            assert info.restart_interval > 0
        got = R.reconstruct(jpeg.entropy_decode(data))
        want = R.pillow_rgb(data)
        assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} bytes differ"


def test_golden_restart_files_equal_pillow_and_the_stored_arrays():
    from wu import jpeg
    with np.load(os.path.join(GOLDEN, "expected.npz")) as exp:
        for name in ("baseline_420.jpg", "restart_blocks.jpg", "restart_rows.jpg", "restart_grey.jpg"):
            data = _golden(name)
            got = R.reconstruct(jpeg.entropy_decode(data))
            assert np.array_equal(got, R.pillow_rgb(data)), name
            assert np.array_equal(got, exp[name]), name
        for name in ("progressive.jpg", "cmyk.jpg", "s440.jpg"):
            with pytest.raises(jpeg.JpegUnsupported):
                jpeg.entropy_decode(_golden(name))
            assert np.array_equal(R.pillow_rgb(_golden(name)), exp[name]), f"{name}: this Pillow decodes the fixture differently"


def test_magnitude_bound_is_reported():
    """Full-swing noise at quality 100 has blocks whose sum |c*q| passes the bound under which the 16-bit IDCT lanes cannot
    saturate (csrc/jpeg.hip kMaxBlockL1): reported as unsupported, not decoded approximately."""
    from wu import _lib, jpeg
    rng = np.random.default_rng(0)
    img = np.repeat((rng.integers(0, 2, (32, 32, 1)) * 255).astype(np.uint8), 3, axis=2)      # black / white noise: luma swings fully
    data = R.encode(img, dict(quality=100, subsampling=0))
    with pytest.raises(jpeg.JpegUnsupported) as e:
        jpeg.entropy_decode(data)
    assert e.value.reason == "magnitude"
    assert 5000 <= _lib.load().wu_jpeg_max_block_l1() <= 5904


# ---- 3. corrupt input -------------------------------------------------------------------------------------------------------------
def test_corrupt_scans_end_with_an_error():
    from wu import jpeg
    data = R.encode(R.synth(97, 131, 2), dict(quality=75))
    scan = jpeg.parse(data).scan_offset
    for cut in (scan + 1, scan + 40, scan + (len(data) - scan) // 2, len(data) - 40):
        with pytest.raises(jpeg.JpegError, match="premature|Huffman|index"):
            jpeg.entropy_decode(data[:cut])
    # truncated, then padded with zeros / with a marker: still an error, never a read past the buffer
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_decode(data[:scan + 100] + b"\xff\xd9")
    rst = _golden("restart_blocks.jpg")
    at = rst.index(b"\xff\xd1")
    with pytest.raises(jpeg.JpegError, match="restart"):
        jpeg.entropy_decode(rst[:at] + b"\xff\xd3" + rst[at + 2:])
    with pytest.raises(jpeg.JpegError, match="restart|premature"):
        jpeg.entropy_decode(rst[:at] + rst[at + 2:])                                   # a restart marker removed


def test_flipped_bytes_in_a_huffman_table_never_crash():
    from wu import jpeg
    data = R.encode(R.synth(64, 48, 4), dict(quality=75))
    dht = data.index(b"\xff\xc4")
    want_shape = [p.shape for p in jpeg.entropy_decode(data)[0]]
    outcomes = set()
    for off in range(5, 60):
        for val in (0x00, 0xFF, data[dht + off] ^ 0x55):
            bad = data[:dht + off] + bytes([val]) + data[dht + off + 1:]
            try:
                planes, _, _ = jpeg.entropy_decode(bad)
                assert [p.shape for p in planes] == want_shape
                outcomes.add("decoded")
            except jpeg.JpegError:
                outcomes.add("error")
            except jpeg.JpegUnsupported as e:
                assert e.reason in ("corrupt-header", "magnitude")
                outcomes.add("unsupported")
    assert "error" in outcomes


def test_coefficient_buffer_capacity_is_checked():
    import ctypes
    from wu import _lib, jpeg
    lib = _lib.load()
    data = R.encode(R.synth(64, 48, 4), dict(quality=75))
    info = jpeg.parse(data)
    coef = np.zeros(info.total_blocks * 64, dtype=np.int16)
    q = np.zeros((3, 64), dtype=np.uint16)
    assert lib.wu_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, coef.nbytes - 2, q.ctypes.data) < 0
    assert b"too small" in lib.wu_last_error() and not coef.any()
    bad = jpeg.parse(_golden("progressive.jpg"))
    assert lib.wu_jpeg_entropy_decode(data, len(data), ctypes.byref(bad), coef.ctypes.data, coef.nbytes, q.ctypes.data) < 0


# ---- 4. loader ----------------------------------------------------------------------------------------------------------------------
class _StubDecoder:
    """prepare / finish of GPUJpegDecoder without a GPU: a 'batch' is the list of its paths."""
    def __init__(self, delay=0.0, fail_at=None):
        self.prepared, self.finished, self.delay, self.fail_at = [], [], delay, fail_at
        self.threads = set()

    def prepare(self, items):
        import time
        self.threads.add(threading.current_thread().name)
        time.sleep(self.delay)
        if self.fail_at is not None and len(self.prepared) == self.fail_at:
            raise RuntimeError("cannot decode image " + items[0])
        self.prepared.append(list(items))
        return list(items)

    def finish(self, hb):
        self.finished.append(hb)
        return torch.zeros((len(hb), 4, 4, 3), dtype=torch.uint8), [(4, 4)] * len(hb)


def _loader_threads():
    return [t for t in threading.enumerate() if t.name == "wu-jpeg-loader"]


def test_loader_order_is_a_pure_function_of_the_arguments():
    from wu.data import JpegBatchLoader
    paths = [f"img{i:03d}.jpg" for i in range(23)]
    labels = np.arange(23) % 5

    def run(**kw):
        ld = JpegBatchLoader(paths, labels, decoder=_StubDecoder(), **kw)
        return [[(p, t.tolist()) for (_, t, p) in ld] for _ in range(2)], ld

    (e0, e1), ld = run(batch_size=4)
    assert [p for p, _ in e0] == [paths[i:i + 4] for i in range(0, 23, 4)] and e0 == e1 and len(ld) == 6
    assert all(t == [int(p[3:6]) % 5 for p in ps] for ps, t in e0)
    (e0, e1), ld = run(batch_size=4, drop_last=True)
    assert len(e0) == 5 == len(ld) and all(len(p) == 4 for p, _ in e0)
    (s0, s1), _ = run(batch_size=5, shuffle=True, seed=3)
    (r0, r1), _ = run(batch_size=5, shuffle=True, seed=3)
    assert s0 == r0 and s1 == r1 and s0 != s1                                             # same seed: same epochs; epochs differ
    assert sorted(p for ps, _ in s0 for p in ps) == paths                                # a permutation
    (o0, _), _ = run(batch_size=5, shuffle=True, seed=4)
    assert o0 != s0
    g = torch.Generator()
    g.manual_seed(3)
    assert [p for ps, _ in s0 for p in ps] == [paths[i] for i in torch.randperm(23, generator=g).tolist()]
    # the stub's prepare ran on the background thread, finish in the consumer's
    ld = JpegBatchLoader(paths, decoder=_StubDecoder(), batch_size=8)
    out = list(ld)
    assert ld.decoder.threads == {"wu-jpeg-loader"} and all(t is None for _, t, _ in out) and len(ld.decoder.finished) == 3
    assert isinstance(out[0][0], tuple) and out[0][0][1] == [(4, 4)] * 8                 # pipeline None: (src_u8, sizes)


def test_loader_weighted_sampling_matches_the_reference_sampler():
    """sampler.py:28-39, 52-54: weights 1 / count[label], torch.multinomial(weights, num_samples, replacement=True)."""
    from wu.data import JpegBatchLoader, class_balanced_weights
    labels = [0] * 40 + [1] * 8 + [2] * 2
    w = class_balanced_weights(labels)
    count = {0: 40, 1: 8, 2: 2}
    assert w == [1.0 / count[x] for x in labels]
    assert class_balanced_weights(torch.tensor(labels)) == w
    paths = [f"{i}.jpg" for i in range(50)]
    ld = JpegBatchLoader(paths, labels, decoder=_StubDecoder(), batch_size=10, sample_weights=w, num_samples=3000, seed=11)
    assert len(ld) == 300
    drawn = [int(p.split(".")[0]) for _, _, ps in ld for p in ps]
    g = torch.Generator()
    g.manual_seed(11)
    assert drawn == torch.multinomial(torch.tensor(w, dtype=torch.float64), 3000, replacement=True, generator=g).tolist()
    per_class = np.bincount([labels[i] for i in drawn], minlength=3) / 3000.0
    assert np.all(np.abs(per_class - 1 / 3) < 0.05)                                      # balanced: 3 sigma of a 1/3 binomial at 3000 draws = 0.026
    assert ld.epoch_indices(0) == drawn and ld.epoch_indices(1) != drawn


def test_loader_shutdown_joins_its_thread():
    from wu.data import JpegBatchLoader
    paths = [f"{i}.jpg" for i in range(200)]
    assert not _loader_threads()
    ld = JpegBatchLoader(paths, decoder=_StubDecoder(delay=0.002), batch_size=4, prefetch=2)
    for k, _ in enumerate(ld):
        if k == 3:
            break
    gc.collect()
    assert not _loader_threads()                                                          # break: the generator's finally joined it
    assert len(ld.decoder.prepared) <= 4 + 2 + 2                                          # it never ran further ahead than prefetch
    it = iter(ld)
    next(it)
    assert len(_loader_threads()) == 1
    ld.close()
    assert not _loader_threads()
    with pytest.raises(ZeroDivisionError):
        for k, _ in enumerate(ld):
            if k == 2:
                1 / 0
    gc.collect()
    assert not _loader_threads()
    # an error on the background thread reaches the consumer, with the file named
    ld = JpegBatchLoader(paths, decoder=_StubDecoder(fail_at=2), batch_size=4)
    with pytest.raises(RuntimeError, match="cannot decode image 8.jpg"):
        list(ld)
    assert not _loader_threads()
    with pytest.raises(ValueError):
        JpegBatchLoader(paths, targets=[0], decoder=_StubDecoder())


# ---- 5. thread safety of the host stage ----------------------------------------------------------------------------------------------
def test_host_stage_is_thread_safe():
    from wu import jpeg
    files = [d for _, d in R.grid([(97, 131), (64, 48), (120, 161), (33, 17), (18, 34)])][:64]
    assert len(files) == 64

    def dec(d):
        planes, q, info = jpeg.entropy_decode(d)
        return [p.copy() for p in planes], q.copy(), info.max_block_l1

    single = [dec(d) for d in files]
    with ThreadPoolExecutor(max_workers=16) as ex:
        for rep in range(3):
            multi = list(ex.map(dec, files))
            for a, b in zip(single, multi):
                assert a[2] == b[2] and np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


# ---- 6. the staging layout prepare() builds (what the kernels will read), checked on the host -------------------------------------------
def test_prepare_lays_out_a_mixed_batch():
    from wu import jpeg
    dec = jpeg.GPUJpegDecoder(threads=4)
    assert 1 <= dec.threads <= 16 and jpeg.GPUJpegDecoder(threads=64).threads == 16
    cases = R.grid([(97, 131), (7, 5), (40, 3)])[:20]
    items = [d for _, d in cases] + [os.path.join(GOLDEN, "progressive.jpg"), os.path.join(GOLDEN, "rgb.png")]
    hb = dec.prepare(items)
    assert dec.stats == {"native": 20, "fallback": 2, "fallback_reasons": {"progressive": 1, "not-jpeg": 1}}
    st, off = hb.staging.array, hb.off
    desc = st[off["desc"]:off["desc"] + hb.n * 64].view(np.int32).reshape(hb.n, 16)
    tile = st[off["tile"]:off["tile"] + hb.n_tiles * 4].view(np.int32)
    coef = st[:hb.n_tiles * 32 * 128].view(np.int16)
    qtab = st[off["qtab"]:off["qtab"] + hb.n * 384].view(np.uint16).reshape(hb.n, 3, 64)
    next_tile = 0
    for i, data in enumerate(items[:20]):
        first_block, h, w, mode, bwy, bhy, bwc, bhc, first_tile, nblocks = desc[i, :10]
        info = jpeg.parse(data)
        assert (h, w, mode) == (info.height, info.width, info.mode) and first_tile == next_tile and first_block == 32 * first_tile
        nt = -(-nblocks // 32)
        assert np.all(tile[first_tile:first_tile + nt] == i)
        next_tile += nt
        planes, at = [], first_block
        for (bw, bh) in [(bwy, bhy)] + ([(bwc, bhc)] * 2 if mode else []):
            planes.append(coef[at * 64:(at + bw * bh) * 64].reshape(bh, bw, 64))
            at += bw * bh
        assert at - first_block == nblocks
        assert np.array_equal(R.reconstruct((planes, qtab[i], info)), R.pillow_rgb(data)), cases[i][0]
    assert next_tile == hb.n_tiles and np.all(desc[20:, 1:8] == 0) and np.all(desc[20:, 9] == 0)
    assert [s for s, _ in hb.fallbacks] == [20, 21] and hb.sizes[20:] == [(52, 70), (52, 70)]
    assert (hb.hmax, hb.wmax) == (97, 131)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.finish(hb)
    # a released buffer is reused, a held one is not
    st0 = hb.staging
    hb2 = dec.prepare(items[:3])
    assert hb2.staging is not st0
    hb.release()
    hb3 = dec.prepare(items[:3])
    assert hb3.staging is st0
    with pytest.raises(RuntimeError, match="truncated.jpg"):
        dec.prepare([items[0], os.path.join(GOLDEN, "truncated.jpg")])
    dec.close()


def test_a_header_claiming_a_huge_image_is_left_to_pillow():
    """No staging memory is sized from an unchecked header: past Pillow's own pixel limit the file is Pillow's to judge."""
    from wu import jpeg
    data = bytearray(R.encode(R.synth(16, 16, 1), dict(quality=75)))
    sof = bytes(data).index(b"\xff\xc0")
    data[sof + 5:sof + 9] = bytes([0x4E, 0x20, 0x4E, 0x20])                        # 20000 x 20000
    info = jpeg.parse(bytes(data))
    assert info.supported == 1 and info.height * info.width > jpeg.MAX_NATIVE_PIXELS
    dec = jpeg.GPUJpegDecoder(threads=1)
    with pytest.raises(RuntimeError, match="cannot decode image <bytes #0>"):
        dec.prepare([bytes(data)])
    assert not dec._staging
    dec.close()
