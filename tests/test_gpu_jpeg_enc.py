"""GPU: the JPEG encoder (wu/jpeg_enc.py, csrc/jpeg_enc.hip) against Pillow -- what the reference's inference scripts run
(inf_transfer_c.py:119-120: save_image(output, '....jpg', normalize=True), one Image.save per image).  Bar: every file equals
Pillow's byte for byte, live and against the stored fixtures; no tolerance anywhere."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_enc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc")


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def _assert_same(got, want, what):
    assert got == want, f"{what}: {len(got)} bytes vs Pillow's {len(want)}, first difference at byte {_first_diff(got, want)}"


@pytest.fixture(scope="module")
def encoders():
    from wu.jpeg_enc import GPUJpegEncoder
    made = {}

    def get(quality=75, subsampling="4:2:0"):
        key = (quality, subsampling)
        if key not in made:
            made[key] = GPUJpegEncoder(DEV, quality=quality, subsampling=subsampling)
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("quality", [75, 100, 30])
def test_single_images_equal_pillow(encoders, quality):
    """One image per batch over the sizes that reach every edge rule -- dummy blocks right and bottom, both chroma padding rules, a
    single row / column of pixels -- times the contents that reach every symbol class (ZRL, no EOB, DC category 11, dense stuffing:
    tests/test_jpeg_enc_cpu.py::test_grid_reaches_the_hard_symbols)."""
    enc = encoders(quality)
    before = enc.stats["native"]
    for h, w in R.GPU_SIZES:
        for content in R.CONTENTS:
            img = R.make_image(h, w, content)
            got = enc.encode_batch(torch.from_numpy(img[None]).to(DEV))
            assert len(got) == 1
            _assert_same(got[0], R.pillow_jpeg(img, quality), f"{h}x{w} {content} q{quality}")
    assert enc.stats["native"] - before == len(R.GPU_SIZES) * len(R.CONTENTS) and enc.stats["fallback"] == 0


def test_444_equals_pillow(encoders):
    for quality in (75, 100):
        enc = encoders(quality, "4:4:4")
        for h, w in [(1, 1), (7, 5), (17, 17), (24, 40), (33, 1), (50, 16)]:
            for content in ("noise", "saturated"):
                img = R.make_image(h, w, content)
                # full-swing content at 4:4:4 and quality 100 takes MORE than its raw size (the default capacity): give it room, so that
                # it is the kernels that are tested here and not the fallback
                got = enc.encode_batch(torch.from_numpy(img[None]).to(DEV), capacity=2 * len(R.encode(img, quality, "4:4:4")))
                _assert_same(got[0], R.pillow_jpeg(img, quality, 0), f"{h}x{w} {content} q{quality} 4:4:4")
        assert enc.stats["fallback"] == 0


def test_fixtures(encoders):
    """The stored Pillow files: pins the bytes whatever Pillow this machine has."""
    stems = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npy"))
    assert len(stems) == 12
    for s in stems:
        _, _, q, sub = s.split("_")
        img = np.load(os.path.join(GOLDEN, s + ".npy"))
        with open(os.path.join(GOLDEN, s + ".jpg"), "rb") as fh:
            want = fh.read()
        enc = encoders(int(q[1:]), {"420": "4:2:0", "444": "4:4:4"}[sub])
        _assert_same(enc.encode_batch(torch.from_numpy(img[None]).to(DEV))[0], want, s)


def test_mixed_batch_with_sizes_never_reads_the_padding(encoders):
    """Eight sizes in one padded (N, Hmax, Wmax, 3) tensor, as GPUJpegDecoder emits it: per-image offsets, and the same files whatever
    the padding holds."""
    enc = encoders()
    sizes = [(1, 1), (7, 5), (16, 16), (17, 17), (24, 40), (40, 24), (33, 1), (50, 16)]
    imgs = [R.make_image(h, w, c) for (h, w), c in zip(sizes, ("noise", "gradient", "flat", "saturated") * 2)]
    hm, wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    results = []
    for fill in (0, 255, None):
        pad = np.random.default_rng(5).integers(0, 256, (len(imgs), hm, wm, 3), dtype=np.uint8) if fill is None else np.full((len(imgs), hm, wm, 3), fill, np.uint8)
        for i, im in enumerate(imgs):
            pad[i, :im.shape[0], :im.shape[1]] = im
        results.append(enc.encode_batch(torch.from_numpy(pad).to(DEV), sizes))
    for files in results:
        assert len(files) == len(imgs)
        for f, im in zip(files, imgs):
            _assert_same(f, R.pillow_jpeg(im), f"{im.shape[0]}x{im.shape[1]} in the mixed batch")
    with pytest.raises(ValueError):
        enc.encode_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV), [(8, 8), (9, 8)])
    with pytest.raises(ValueError):
        enc.encode_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV), [(8, 8)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
def test_float_batches_equal_encoding_to_uint8(encoders, dtype, channels_last):
    """(4, 3, 64, 64) floats, some outside [0, 1]: the encoder's own conversion is wu.infer_driver.to_uint8's, in either memory format."""
    from wu.infer_driver import to_uint8
    x = (torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 1.2 - 0.1).to(dtype).to(DEV)
    x[0, :, :4, :4] = torch.tensor([0.0, 1.0, 0.5, 1.0 / 255, 254.999 / 255, 2.0 / 255, -0.0, 1e-9, 0.999, 128 / 255, 0.25, 0.75, 255.5 / 255, -1.0, 3.0, 0.1],
                                   device=DEV).to(dtype).view(4, 4)
    want = to_uint8(x).cpu().numpy()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
        assert not x.is_contiguous()
    enc = encoders()
    files = enc.encode_batch(x)
    via_u8 = enc.encode_batch(torch.from_numpy(want).to(DEV))
    for i in range(4):
        _assert_same(files[i], R.pillow_jpeg(want[i]), f"float image {i}")
        assert files[i] == via_u8[i]


@pytest.mark.parametrize("size", [224, 512])
def test_prefix_sum_across_workgroups(encoders, size):
    """224^2 has 1176 blocks, 512^2 6144: 5 and 24 tiles of the bit-offset prefix sum, several 4 KiB chunks of the stuffing one."""
    enc = encoders()
    img = R.make_image(size, size, "noise")
    _assert_same(enc.encode_batch(torch.from_numpy(img[None]).to(DEV))[0], R.pillow_jpeg(img), f"{size}^2 noise")


def test_kernel_stages_equal_the_restatement(encoders):
    """Coefficients, per-block bit offsets and the raw bit stream out of the workspace, against tests/_jpeg_enc_ref.stages: a file
    mismatch elsewhere can be pinned to its kernel from here."""
    from wu import _lib
    from wu.jpeg_enc import SUBSAMPLING
    lib = _lib.load()
    for (h, w), sub in (((50, 16), "4:2:0"), ((17, 17), "4:2:0"), ((100, 75), "4:2:0"), ((24, 40), "4:4:4")):
        img = R.make_image(h, w, "noise")
        enc = encoders(75, sub)
        res = enc.launch(torch.from_numpy(img[None]).to(DEV))
        st = R.stages(img, 75, sub)
        lay = (ctypes.c_longlong * 8)()
        assert lib.wu_jpeg_enc_workspace_layout(1, h, w, SUBSAMPLING[sub], res.plan.cap_max, lay) == 0
        ws = res.workspace.cpu().numpy()
        nb = len(st["blocks"])
        coef = ws[lay[0]:lay[0] + nb * 128].view(np.int16).reshape(nb, 64)
        assert np.array_equal(coef, st["blocks"]), f"{h}x{w} {sub}: blocks {np.flatnonzero((coef != st['blocks']).any(axis=1))[:8]} differ"
        off = ws[lay[1]:lay[1] + nb * 4].view(np.uint32).astype(np.int64)
        tiles = ws[lay[2]:lay[2] + (nb + 255) // 256 * 4].view(np.uint32).astype(np.int64)
        base = np.concatenate([[0], np.cumsum(tiles)])[np.arange(nb) // 256]
        assert np.array_equal(off + base, np.concatenate([[0], np.cumsum(st["bits"])])[:nb])
        assert tiles.sum() == st["bits"].sum()
        assert bytes(ws[lay[4]:lay[4] + len(st["raw"])]) == st["raw"]
        assert res.result.cpu().tolist() == [[len(st["file"]), 0]]


def test_overflow_falls_back_to_pillow_and_is_counted():
    from wu.jpeg_enc import GPUJpegEncoder
    enc = GPUJpegEncoder(DEV, quality=100)
    imgs = np.stack([R.make_image(64, 64, "noise"), R.make_image(64, 64, "flat"), R.make_image(64, 64, "noise", seed=1)])
    x = torch.from_numpy(imgs).to(DEV)
    res = enc.launch(x, capacity=2048)                   # 64^2 noise at quality 100 takes ~8 KB, the flat image a few dozen bytes
    assert res.result.cpu()[:, 1].tolist() == [1, 0, 1] and res.result.cpu()[0, 0].item() == 0       # flagged, not truncated
    files = enc.fetch(res)
    for f, im in zip(files, imgs):
        _assert_same(f, R.pillow_jpeg(im, 100), "overflow batch")
    assert enc.stats == {"native": 1, "fallback": 2, "fallback_reasons": {"capacity": 2}}
    # the stuffed stream alone can be what does not fit: saturated content is dense in 0xFF
    sat = R.make_image(64, 48, "saturated")
    st = R.stages(sat, 100)
    assert len(st["scan"]) > len(st["raw"])
    files = enc.encode_batch(torch.from_numpy(sat[None]).to(DEV), capacity=len(st["raw"]))
    _assert_same(files[0], R.pillow_jpeg(sat, 100), "stuffing overflow")
    assert enc.stats["fallback"] == 3
    files = enc.encode_batch(torch.from_numpy(sat[None]).to(DEV), capacity=len(st["scan"]))          # exactly enough: native
    _assert_same(files[0], R.pillow_jpeg(sat, 100), "exact capacity")
    assert enc.stats["fallback"] == 3 and enc.stats["native"] == 2
    # float input through the fallback
    xf = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    from wu.infer_driver import to_uint8
    _assert_same(enc.encode_batch(xf, capacity=64)[0], R.pillow_jpeg(to_uint8(xf).cpu().numpy()[0], 100), "float fallback")
    assert enc.stats["fallback"] == 4
    enc.close()


def test_launch_in_a_captured_graph_replays_over_new_pixels(encoders, monkeypatch):
    enc = encoders()
    a, b = R.make_image(40, 56, "gradient"), R.make_image(40, 56, "noise")
    x = torch.from_numpy(np.stack([a, b])).to(DEV)
    enc.launch(x)                                        # uploads this geometry's descriptors and headers
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # five kernels, a plain linear chain
        res = enc.launch(x)
    for pair in ((b, a), (R.make_image(40, 56, "saturated"), R.make_image(40, 56, "flat")), (a, b)):
        x.copy_(torch.from_numpy(np.stack(pair)).to(DEV))
        graph.replay()
        files = enc.fetch(res)
        for f, im in zip(files, pair):
            _assert_same(f, R.pillow_jpeg(im), "graph replay")
    # a geometry that was never launched cannot be captured (its descriptors would have to be uploaded inside the capture): said, not tried
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="outside the capture"):
        enc.launch(torch.zeros(1, 24, 8, 3, dtype=torch.uint8, device=DEV))


def test_save_images_and_class_sweep_to_dir(tmp_path, encoders):
    """The drivers' last line: file names of inf_transfer_c.py:119-120, Pillow's bytes, and the round trip through GPUJpegDecoder."""
    from PIL import Image
    import cunet
    from oracle import cunet_ref as O
    from wu.infer_driver import class_sweep, class_sweep_to_dir, normalize_minmax, save_images, to_uint8
    from wu.jpeg import GPUJpegDecoder
    nc = 3
    x, _ = O.make_inputs(2, 64, nc, 0, False)
    net = cunet.Conditional_UNet(nc, precision="fp32")
    net.load_state_dict(O.make_cunet_params(nc, 0))
    net = net.to(DEV).eval()
    batch = x.to(DEV)
    names = ["sunny", "cloudy", "rain"]
    out_dir = str(tmp_path / "sweep")
    paths = class_sweep_to_dir(net, batch, ["img0001", "b"], [2, 0], names, out_dir)
    assert [os.path.basename(p) for p in paths] == [f"{s}_{t}.jpg" for t in names for s in ("rain_img0001", "sunny_b")]
    assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths)
    want_u8 = to_uint8(class_sweep(net, batch, nc, normalize=True).flatten(0, 1)).cpu().numpy()          # (nc * B, H, W, 3), target-major
    for p, rgb in zip(paths, want_u8):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "JPEG")
        with open(p, "rb") as fh:
            _assert_same(fh.read(), buf.getvalue(), os.path.basename(p))
    dec = GPUJpegDecoder(DEV)
    src, sizes = dec.decode_batch(paths)
    assert sizes == [(64, 64)] * len(paths) and dec.stats["fallback"] == 0
    got = src.cpu().numpy()
    for i, p in enumerate(paths):
        assert np.array_equal(got[i], np.array(Image.open(p).convert("RGB"))), os.path.basename(p)
    dec.close()
    # save_images alone: raw network outputs, mixed extensions, an explicit encoder
    y = net(batch, torch.eye(nc, device=DEV)[[1, 1]])
    mixed = [str(tmp_path / "a.JPG"), str(tmp_path / "b.png")]
    save_images(y, mixed, normalize=True, encoder=encoders(75, "4:2:0"))
    rgb = to_uint8(normalize_minmax(y)).cpu().numpy()
    buf = io.BytesIO()
    Image.fromarray(rgb[0]).save(buf, "JPEG")
    with open(mixed[0], "rb") as fh:
        _assert_same(fh.read(), buf.getvalue(), "a.JPG")
    assert np.array_equal(np.array(Image.open(mixed[1])), rgb[1])                                        # PNG: lossless, written by Pillow
    with pytest.raises(ValueError):
        save_images(y, mixed[:1])
