"""GPU: the PNG encoder (wu/png_enc.py, csrc/png_enc.hip).  PNG is lossless and Pillow runs zlib's matcher, so Pillow's bytes are not
the bar.  The bar: every file equals the CPU restatement (tests/_png_enc_ref.py, itself validated by tests/test_png_enc_cpu.py) byte
for byte, and decodes in Pillow -- which checks every CRC and the Adler-32 -- to the input pixels; no tolerance anywhere."""
import io
import os

import numpy as np
import pytest
import torch

import _png_enc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def _assert_same(got, want, what):
    assert got == want, f"{what}: {len(got)} bytes vs the restatement's {len(want)}, first difference at byte {_first_diff(got, want)}"


def _decode(data):
    from PIL import Image
    Image.open(io.BytesIO(data)).verify()
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB"
    return np.asarray(im)


@pytest.fixture(scope="module")
def enc():
    from wu.png_enc import GPUPngEncoder
    e = GPUPngEncoder(DEV)
    yield e
    e.close()


@pytest.fixture(scope="module")
def grid():
    """(image, the restatement's file) per case, computed once."""
    out = {}
    for case in R.GRID:
        img = R.make_image(*case)
        out[case] = (img, R.encode(img))
    return out


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_single_images_equal_the_restatement_and_decode(enc, grid, case):
    img, want = grid[case]
    before = enc.stats["native"]
    got = enc.encode_batch(torch.from_numpy(img[None]).to(DEV))
    assert len(got) == 1 and enc.stats["native"] == before + 1
    assert np.array_equal(_decode(got[0]), img), R.case_id(case)
    _assert_same(got[0], want, R.case_id(case))
    assert len(got[0]) <= R.out_stride(case[0], case[1])


def test_mixed_batch_with_sizes_never_reads_the_padding(enc, grid):
    """Every case of the grid in one padded (N, Hmax, Wmax, 3) tensor: per-image segment counts and offsets, and the same files
    whatever the padding holds."""
    cases = list(R.GRID)
    sizes = [(c[0], c[1]) for c in cases]
    hm, wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    for fill in (0, None):
        pad = np.random.default_rng(5).integers(0, 256, (len(cases), hm, wm, 3), dtype=np.uint8) if fill is None else np.full((len(cases), hm, wm, 3), fill, np.uint8)
        for i, c in enumerate(cases):
            pad[i, :c[0], :c[1]] = grid[c][0]
        files = enc.encode_batch(torch.from_numpy(pad).to(DEV), sizes)
        assert len(files) == len(cases)
        for f, c in zip(files, cases):
            _assert_same(f, grid[c][1], f"{R.case_id(c)} in the mixed batch")
    with pytest.raises(ValueError):
        enc.encode_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV), [(8, 8), (9, 8)])
    with pytest.raises(ValueError):
        enc.encode_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV), [(8, 8)])


@pytest.mark.parametrize("layout", ["fp32", "bf16", "channels_last", "strided_slice"])
def test_float_batches_equal_encoding_to_uint8(enc, layout):
    """(3, 3, 48, 72) floats (a 40 x 28 window of them for the slice), some outside [0, 1]: the encoder's own conversion is wu.infer_driver.to_uint8's, whatever the strides."""
    from wu.infer_driver import to_uint8
    dtype = torch.bfloat16 if layout == "bf16" else torch.float32
    x = (torch.rand(3, 3, 48, 72, generator=torch.Generator().manual_seed(3)) * 1.2 - 0.1).to(dtype).to(DEV)
    x[0, :, :4, :4] = torch.tensor([0.0, 1.0, 0.5, 1.0 / 255, 254.999 / 255, 2.0 / 255, -0.0, 1e-9, 0.999, 128 / 255, 0.25, 0.75, 255.5 / 255, -1.0, 3.0, 0.1],
                                   device=DEV).to(dtype).view(4, 4)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
        assert not x.is_contiguous()
    if layout == "strided_slice":
        x = x[:, :, 3:43, 5:61:1][:, :, :, ::2]                       # rows and columns of a larger tensor, every second column
        assert not x.is_contiguous() and x.stride(3) == 2
    want = to_uint8(x).cpu().numpy()
    files = enc.encode_batch(x)
    via_u8 = enc.encode_batch(torch.from_numpy(want).to(DEV))
    for i in range(x.shape[0]):
        assert np.array_equal(_decode(files[i]), want[i])
        _assert_same(files[i], R.encode(want[i]), f"{layout} image {i}")
        assert files[i] == via_u8[i]


def test_two_launches_give_identical_bytes(enc, grid):
    imgs = np.stack([grid[(75, 100, "gradient_noise")][0], R.make_image(75, 100, "natural")])
    x = torch.from_numpy(imgs).to(DEV)
    a, b = enc.launch(x), enc.launch(x)
    fa, fb = enc.fetch(a), enc.fetch(b)
    assert fa == fb and fa[0] == grid[(75, 100, "gradient_noise")][1]


def test_launch_in_a_captured_graph_replays_over_new_pixels(enc, monkeypatch):
    a, b = R.make_image(40, 56, "gradient_noise"), R.make_image(40, 56, "noise")
    x = torch.from_numpy(np.stack([a, b])).to(DEV)
    eager = enc.encode_batch(x)                          # uploads this geometry's descriptors
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # three kernels, a plain linear chain
        res = enc.launch(x)
    graph.replay()
    assert enc.fetch(res) == eager
    for pair in ((b, a), (R.make_image(40, 56, "saturated"), R.make_image(40, 56, "flat"))):
        x.copy_(torch.from_numpy(np.stack(pair)).to(DEV))
        graph.replay()
        for f, im in zip(enc.fetch(res), pair):
            _assert_same(f, R.encode(im), "graph replay")
    # a geometry that was never launched cannot be captured (its descriptors would have to be uploaded inside the capture): said, not tried
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="outside the capture"):
        enc.launch(torch.zeros(1, 24, 8, 3, dtype=torch.uint8, device=DEV))


def test_save_images_and_class_sweep_to_dir(tmp_path, enc):
    from PIL import Image
    import cunet
    from oracle import cunet_ref as O
    from wu.infer_driver import class_sweep, class_sweep_to_dir, normalize_minmax, save_images, to_uint8
    from wu.jpeg_enc import GPUJpegEncoder
    nc = 3
    x, _ = O.make_inputs(2, 64, nc, 0, False)
    net = cunet.Conditional_UNet(nc, precision="fp32")
    net.load_state_dict(O.make_cunet_params(nc, 0))
    net = net.to(DEV).eval()
    batch = x.to(DEV)
    names = ["sunny", "cloudy", "rain"]
    # save_images: mixed extensions, both encoders
    y = net(batch, torch.eye(nc, device=DEV)[[1, 1]])
    mixed = [str(tmp_path / "a.JPG"), str(tmp_path / "b.png")]
    jenc = GPUJpegEncoder(DEV)
    before = enc.stats["native"]
    save_images(y, mixed, normalize=True, encoder=jenc, png_encoder=enc)
    jenc.close()
    rgb = to_uint8(normalize_minmax(y)).cpu().numpy()
    buf = io.BytesIO()
    Image.fromarray(rgb[0]).save(buf, "JPEG")
    with open(mixed[0], "rb") as fh:
        assert fh.read() == buf.getvalue()                             # the JPEG still Pillow's bytes
    with open(mixed[1], "rb") as fh:
        data = fh.read()
    _assert_same(data, R.encode(rgb[1]), "b.png")
    assert np.array_equal(_decode(data), rgb[1]) and enc.stats["native"] == before + 1
    # class_sweep_to_dir with the encoder
    out_dir = str(tmp_path / "sweep")
    paths = class_sweep_to_dir(net, batch, ["img0001", "b"], [2, 0], names, out_dir, ext=".png", png_encoder=enc)
    assert [os.path.basename(p) for p in paths] == [f"{s}_{t}.png" for t in names for s in ("rain_img0001", "sunny_b")]
    assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths)
    want_u8 = to_uint8(class_sweep(net, batch, nc, normalize=True).flatten(0, 1)).cpu().numpy()          # (nc * B, H, W, 3), target-major
    for p, want in zip(paths, want_u8):
        with open(p, "rb") as fh:
            data = fh.read()
        assert np.array_equal(_decode(data), want), os.path.basename(p)
        assert R.unpack(data)[:2] == (64, 64)
    assert enc.stats["native"] == before + 1 + len(paths)
    # ... and without it: Pillow's own bytes, as before
    plain_dir = str(tmp_path / "plain")
    plain = class_sweep_to_dir(net, batch, ["img0001", "b"], [2, 0], names, plain_dir, ext=".png")
    for p, want in zip(plain, want_u8):
        buf = io.BytesIO()
        Image.fromarray(want).save(buf, "PNG")
        with open(p, "rb") as fh:
            assert fh.read() == buf.getvalue(), os.path.basename(p)
    assert enc.stats["native"] == before + 1 + len(paths)
