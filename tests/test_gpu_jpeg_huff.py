"""GPU: the device Huffman decoder (csrc/jpeg_huff.hip, wu.jpeg.GPUJpegDecoder(entropy="device")).  Bar: status 0 and every int16
coefficient and quantisation table equal to the host decoder's (wu.jpeg.entropy_decode); batches byte-equal to the host-mode decoder's
and to Pillow's.  The coefficient buffer carries 32 guard blocks of 0x7777 in front of, between and behind the images, and they must be
intact after every call.  The corrupt inputs used here (truncated.jpg, the over-the-bound noise image) are among the files the sanitizer
emulation (scratch/jpeg_huff_emu.cpp) decodes: they test rejection, nothing is to fault."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
GUARD = 32
SIZES = [(1, 1), (8, 8), (16, 16), (33, 17), (97, 131)]
RESTART = ["restart_blocks.jpg", "restart_rows.jpg", "restart_grey.jpg"]
EDGE_SIZES = [(1, 1), (7, 5), (8, 8), (3, 40), (40, 3), (17, 33), (5, 3), (9, 4), (2, 2), (16, 16), (8, 16), (16, 8), (33, 1)]


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def _noise():
    """Black/white pixel noise at quality 100: a block's sum |c * q| is over the IDCT's overflow bound."""
    img = (np.random.default_rng(7).integers(0, 2, (64, 64, 1)) * 255).astype(np.uint8).repeat(3, 2)
    return R.encode(img, dict(quality=100, subsampling=0))


@pytest.fixture(scope="module")
def host():
    """file bytes -> (flat int16 coefficients, qtabs) of the host decoder, computed once per file (R.grid seeds an image by its place
    in the size list, so a name alone does not identify it)."""
    from wu import jpeg
    out = {}

    def get(name, data):
        if data not in out:
            planes, qt, _ = jpeg.entropy_decode(data)
            out[data] = (np.concatenate([p.reshape(-1) for p in planes]), qt)
        return out[data]
    return get


def _decode_abi(cases, S):
    """wu_jpeg_huff_decode on buffers the test lays out itself.  Returns (status (N,), [coefficients per image], [qtab per image])."""
    from wu import _lib, jpeg
    staged = [jpeg.scan_stage(d, S) for _, d in cases]
    n = len(cases)
    hdesc = np.zeros((n, 16), np.int32)
    scan_at = seg_at = 0
    blocks = GUARD
    for i, st in enumerate(staged):
        info = st["info"]
        hdesc[i, :13] = (scan_at, len(st["scan"]), seg_at, len(st["segs"]), st["n_subseq"], blocks, info.total_blocks, info.ncomp, info.hs[0],
                         info.vs[0], info.mcus_x, info.mcus_x * info.mcus_y, info.restart_interval)
        scan_at += len(st["scan"])
        seg_at += len(st["segs"])
        blocks += info.total_blocks + GUARD
    scan = torch.from_numpy(np.concatenate([st["scan"] for st in staged])).to(DEV)
    segs = torch.from_numpy(np.concatenate([st["segs"] for st in staged])).to(DEV)
    dht = torch.from_numpy(np.concatenate([st["dht"] for st in staged])).to(DEV)
    qtab = torch.from_numpy(np.concatenate([st["qtab"].reshape(-1) for st in staged]).view(np.int16)).to(DEV)
    coef = torch.full((blocks * 64,), 0x7777, dtype=torch.int16, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    hd = torch.from_numpy(hdesc).to(DEV)
    _lib.call("wu_jpeg_huff_decode", scan.data_ptr(), segs.data_ptr(), dht.data_ptr(), hd.data_ptr(), qtab.data_ptr(), coef.data_ptr(),
              status.data_ptr(), n, S, torch.cuda.current_stream().cuda_stream)
    got = coef.cpu().numpy()
    owned = np.zeros(blocks * 64, bool)
    out = []
    for i, st in enumerate(staged):
        a, b = hdesc[i, 5] * 64, (hdesc[i, 5] + hdesc[i, 6]) * 64
        owned[a:b] = True
        out.append(got[a:b])
    guards = got[~owned]
    assert guards.size == (n + 1) * GUARD * 64 and (guards == 0x7777).all(), f"{np.count_nonzero(guards != 0x7777)} guard coefficients overwritten"
    return status.cpu().numpy(), out, [st["qtab"] for st in staged]


def _assert_equal_host(cases, status, coefs, qtabs, host):
    assert (status == 0).all(), [(cases[i][0], hex(int(s))) for i, s in enumerate(status) if s]
    for (name, data), got, qt in zip(cases, coefs, qtabs):
        want, wq = host(name, data)
        assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} of {want.size} coefficients differ"
        assert np.array_equal(qt, wq), name


def test_coefficients_equal_the_host_decoder_at_the_default_subsequence(host):
    from wu import jpeg
    cases = R.grid(R.SMALL_SIZES) + [(n, _golden(n)) for n in RESTART]
    status, coefs, qtabs = _decode_abi(cases, jpeg.DEFAULT_SUBSEQ_BITS)
    _assert_equal_host(cases, status, coefs, qtabs, host)


@pytest.mark.parametrize("S", [64, 128])
def test_coefficients_equal_the_host_decoder_at_short_subsequences(host, S):
    """Scans shorter than one subsequence (1x1), one-MCU images, one-MCU restart segments (q30_444_rst1), and more than one chunk with
    exact carry: 97x131 q100 4:4:4 is over 5000 subsequences at S = 64, with chunks that need every round."""
    from wu import jpeg
    cases = R.grid(SIZES)
    worst = jpeg.scan_stage(dict(cases)["97x131_q100_444"], 64)
    tiny = [jpeg.scan_stage(d, S) for n, d in cases if n.startswith("1x1_")]
    assert worst["n_subseq"] > 5000 and min(int(t["segs"][0, 1]) for t in tiny) < S and min(t["n_subseq"] for t in tiny) == 1
    status, coefs, qtabs = _decode_abi(cases, S)
    _assert_equal_host(cases, status, coefs, qtabs, host)


def test_rejection_leaves_the_neighbours_exact(host):
    from wu import jpeg
    good = R.grid([(97, 131)], R.VARIANTS[:2])
    cases = [good[0], ("truncated.jpg", _golden("truncated.jpg")), good[1]]
    for S in (128, jpeg.DEFAULT_SUBSEQ_BITS):
        status, coefs, qtabs = _decode_abi(cases, S)
        assert status[1] != 0 and status[1] & ~0xFF and jpeg.huff_status_name(status[1]) == "corrupt-scan"
        _assert_equal_host([cases[0], cases[2]], status[[0, 2]], [coefs[0], coefs[2]], [qtabs[0], qtabs[2]], host)


def test_magnitude_bound_is_reported_and_decoded_by_pillow():
    from wu import _lib, jpeg
    data = _noise()
    with pytest.raises(jpeg.JpegUnsupported, match="magnitude") as e:
        jpeg.entropy_decode(data)                                      # the host's A is over 5900
    assert int(str(e.value).rsplit(" ", 1)[1]) > _lib.load().wu_jpeg_max_block_l1() == 5900
    good = R.grid([(33, 17)], R.VARIANTS[:1])[0]
    status, _, _ = _decode_abi([good, ("noise", data)], jpeg.DEFAULT_SUBSEQ_BITS)
    assert list(status) == [0, 11]                                     # WU_JPEG_MAGNITUDE
    dec = jpeg.GPUJpegDecoder(DEV, entropy="device")
    src, sizes, names = dec.decode_batch([good[1], data], return_status=True)
    assert names == ["ok", "magnitude"] and dec.stats == {"native": 1, "fallback": 1, "fallback_reasons": {"magnitude": 1}}
    _check(src, sizes, [good[1], data])
    dec.close()


def _check(src_u8, sizes, datas, names=None):
    out = src_u8.cpu().numpy()
    assert out.shape[0] == len(datas) and out.shape[3] == 3 and out.dtype == np.uint8
    assert out.shape[1] == max(h for h, _ in sizes) and out.shape[2] == max(w for _, w in sizes)
    for i, d in enumerate(datas):
        ref = R.pillow_rgb(d)
        h, w = ref.shape[:2]
        name = names[i] if names else i
        assert tuple(sizes[i]) == (h, w), name
        got = out[i, :h, :w]
        assert np.array_equal(got, ref), f"{name}: {np.count_nonzero(got != ref)} of {ref.size} bytes differ"
        pad = out[i].copy()
        pad[:h, :w] = 0
        assert not pad.any(), f"{name}: {np.count_nonzero(pad)} non-zero padding bytes"


def test_decode_batch_device_entropy_equals_host_mode_and_pillow():
    from wu.jpeg import GPUJpegDecoder
    cases = R.grid(R.SMALL_SIZES) + R.grid(R.LARGE_SIZES, [v for v in R.VARIANTS
                                                            if v[0] in ("q85_420", "q95_422", "q100_444", "q30_rst3", "q75_rstrow", "grey")])
    cases += [(n, _golden(n)) for n in RESTART]
    assert len(cases) >= 150
    datas = [d for _, d in cases]
    dev, hst = GPUJpegDecoder(DEV, entropy="device"), GPUJpegDecoder(DEV)
    src, sizes, names = dev.decode_batch(datas, return_status=True)
    want, wsizes = hst.decode_batch(datas)
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    assert sizes == wsizes and torch.equal(src, want)
    _check(src, sizes, datas, [n for n, _ in cases])
    assert names == ["ok"] * len(cases) and dev.stats["fallback"] == 0 and dev.stats["native"] == len(cases)
    hb = dev.prepare(datas)                                            # the same HostBatch finished twice
    a, _ = dev.finish(hb)
    b, _ = dev.finish(hb)
    hb.release()
    assert torch.equal(a, want) and torch.equal(b, want) and dev.stats["native"] == 2 * len(cases)
    with pytest.raises(ValueError):
        dev.decode_batch([])
    dev.close()
    hst.close()


@pytest.mark.parametrize("size", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_sizes_one_image_per_batch(size):
    from wu.jpeg import GPUJpegDecoder
    dec = GPUJpegDecoder(DEV, threads=2, entropy="device")
    for name, data in R.grid([size]):
        src, sizes = dec.decode_batch([data])
        assert tuple(src.shape) == (1, size[0], size[1], 3)
        _check(src, sizes, [data], [name])
    assert dec.stats["fallback"] == 0
    dec.close()


def test_parser_fallbacks_in_a_device_entropy_batch():
    from wu.jpeg import GPUJpegDecoder
    native = R.grid([(64, 48), (97, 131)], R.VARIANTS[:2])
    fixtures = ["progressive.jpg", "cmyk.jpg", "rgb.png"]
    datas = [native[0][1], _golden(fixtures[0]), native[1][1], _golden(fixtures[1]), native[2][1], _golden(fixtures[2]), native[3][1]]
    dev, hst = GPUJpegDecoder(DEV, entropy="device", subseq_bits=256), GPUJpegDecoder(DEV)
    src, sizes, names = dev.decode_batch(datas, return_status=True)
    want, wsizes = hst.decode_batch(datas)
    assert sizes == wsizes and torch.equal(src, want)
    _check(src, sizes, datas)
    assert names == ["ok", "progressive", "ok", "colorspace", "ok", "not-jpeg", "ok"]
    assert dev.stats == hst.stats == {"native": 4, "fallback": 3, "fallback_reasons": {"progressive": 1, "colorspace": 1, "not-jpeg": 1}}
    with np.load(os.path.join(GOLDEN, "expected.npz")) as exp:          # and the arrays Pillow decoded where the fixtures were written
        for f in fixtures:
            i = datas.index(_golden(f))
            h, w = exp[f].shape[:2]
            assert np.array_equal(src[i, :h, :w].cpu().numpy(), exp[f]), f
    src, sizes = dev.decode_batch([_golden("rgb.png")])                # a batch with no native image at all
    _check(src, sizes, [_golden("rgb.png")])
    with pytest.raises(RuntimeError, match="truncated"):               # the device rejects it, Pillow (the arbiter) cannot read it either
        dev.decode_batch([native[0][1], os.path.join(GOLDEN, "truncated.jpg")])
    dev.close()
    hst.close()


def test_loader_and_fid_take_the_device_entropy_decoder(tmp_path):
    """JpegBatchLoader(decoder=...) and `python -m wu.fid --gpu-entropy`: the same uint8 batches, hence the same results."""
    import _inception_ref as IRF
    from PIL import Image
    from wu.data import JpegBatchLoader
    from wu.fid import statistics_of_path
    from wu.inception import InceptionV3
    from wu.jpeg import GPUJpegDecoder
    d = tmp_path / "imgs"
    d.mkdir()
    for k in range(6):
        Image.fromarray(R.synth(96, 128, 40 + k)).save(d / f"img_{k:02d}.jpg", quality=90 if k % 2 else 75, subsampling=k % 3)
    model = InceptionV3([0])
    model.load_state_dict(IRF.make_params(True, seed=6))
    mu0, sig0 = statistics_of_path(str(d), model, 4, gpu_decode=True)
    mu1, sig1 = statistics_of_path(str(d), model, 4, gpu_entropy=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sig0, sig1)
    files = sorted(str(p) for p in d.glob("*.jpg"))
    dec = GPUJpegDecoder(DEV, entropy="device")
    loader = JpegBatchLoader(files, list(range(6)), batch_size=4, decoder=dec, prefetch=2)
    seen = 0
    for (src, sizes), targets, paths in loader:
        _check(src, sizes, [open(p, "rb").read() for p in paths], paths)
        seen += len(paths)
    assert seen == 6 and dec.stats["fallback"] == 0
    loader.close()
