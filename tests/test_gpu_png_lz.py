"""GPU: the PNG encoder's LZ77 mode (GPUPngEncoder(matching="lz77"), csrc/png_enc.hip).  Every file equals the CPU restatement
(tests/_png_lz_ref.py, itself held to Pillow, zlib and the independent inflate by tests/test_png_lz_cpu.py) byte for byte and decodes
to the input pixels, in Pillow and in the project's own device decoder; no tolerance anywhere.  The default mode did not move."""
import io

import numpy as np
import pytest
import torch

import _png_enc_ref as R
import _png_lz_cases as C
import _png_lz_ref as L

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
    e = GPUPngEncoder(DEV, matching="lz77")
    yield e
    e.close()


@pytest.fixture(scope="module")
def single(enc):
    """name -> the device's file of the case encoded alone, computed once."""
    return {name: enc.encode_batch(torch.from_numpy(C.computed(name)[0][None]).to(DEV))[0] for name in C.NAMES}


@pytest.mark.parametrize("name", C.NAMES)
def test_single_images_equal_the_restatement_and_decode(single, name):
    img, st, lit = C.computed(name)
    assert np.array_equal(_decode(single[name]), img), name
    _assert_same(single[name], st["file"], name)
    assert len(single[name]) <= len(lit) <= R.out_stride(*img.shape[:2])


def test_stats_count_the_segments_by_mode():
    from wu.png_enc import GPUPngEncoder
    e = GPUPngEncoder(DEV, matching="lz77")
    want = {"stored": 0, "literal": 0, "lz77": 0}
    for name in ("99x110_gradient_noise", "128x86_flat", "64x64_noise"):
        img, st, _ = C.computed(name)
        e.encode_batch(torch.from_numpy(img[None]).to(DEV))
        for m in st["modes"]:
            want[{L.STORED: "stored", L.LITERAL: "literal", L.LZ77: "lz77"}[m]] += 1
    e.close()
    assert {k: e.stats[k] for k in want} == want and e.stats["native"] == 3 and min(want.values()) > 0


def test_mixed_batch_with_sizes_never_reads_the_padding(enc, single):
    """Every case in one padded (N, Hmax, Wmax, 3) tensor with poisoned padding: per-image segment counts, row strides and offsets."""
    sizes = [C.computed(n)[0].shape[:2] for n in C.NAMES]
    hm, wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    pad = np.random.default_rng(5).integers(0, 256, (len(C.NAMES), hm, wm, 3), dtype=np.uint8)
    for i, n in enumerate(C.NAMES):
        img = C.computed(n)[0]
        pad[i, :img.shape[0], :img.shape[1]] = img
    files = enc.encode_batch(torch.from_numpy(pad).to(DEV), [tuple(s) for s in sizes])
    assert len(files) == len(C.NAMES)
    for f, n in zip(files, C.NAMES):
        _assert_same(f, single[n], f"{n} in the mixed batch")


@pytest.mark.parametrize("layout", ["fp32", "bf16", "channels_last", "strided_slice"])
def test_float_batches_equal_encoding_to_uint8(enc, layout):
    """The clipped ramp as floats in [0, 1] (a window of a larger tensor for the slice): the conversion in front of the matcher is
    wu.infer_driver.to_uint8's, whatever the precision and the strides."""
    from wu.infer_driver import to_uint8
    img = C.computed("40x64_ramp_clipped")[0]
    dtype = torch.bfloat16 if layout == "bf16" else torch.float32
    x = (torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255).to(dtype).to(DEV)
    if layout == "channels_last":
        x = x.expand(2, -1, -1, -1).contiguous(memory_format=torch.channels_last)
        assert not x.is_contiguous()
    if layout == "strided_slice":
        big = torch.rand(1, 3, 50, 140, device=DEV)
        big[:, :, 5:45, 6:134:2] = x
        x = big[:, :, 5:45, 6:134:2]
        assert not x.is_contiguous() and x.stride(3) == 2
    want = to_uint8(x).cpu().numpy()
    files = enc.encode_batch(x)
    via_u8 = enc.encode_batch(torch.from_numpy(want).to(DEV))
    for i in range(x.shape[0]):
        assert np.array_equal(_decode(files[i]), want[i])
        _assert_same(files[i], L.encode(want[i]), f"{layout} image {i}")
        assert files[i] == via_u8[i]


def test_two_launches_give_identical_bytes(enc, single):
    names = ["grid_3x3_of_24", "102x100_noise_rows_copied"]
    imgs = [C.computed(n)[0] for n in names]
    hm, wm = max(i.shape[0] for i in imgs), max(i.shape[1] for i in imgs)
    x = torch.zeros(2, hm, wm, 3, dtype=torch.uint8, device=DEV)
    for k, im in enumerate(imgs):
        x[k, :im.shape[0], :im.shape[1]] = torch.from_numpy(im).to(DEV)
    sizes = [im.shape[:2] for im in imgs]
    a, b = enc.launch(x, sizes), enc.launch(x, sizes)
    fa, fb = enc.fetch(a), enc.fetch(b)
    assert fa == fb and fa == [single[n] for n in names]


def test_launch_in_a_captured_graph_replays_over_new_pixels(enc):
    a, b = C.computed("40x64_ramp_clipped")[0], R.make_image(40, 64, "noise")
    x = torch.from_numpy(np.stack([a, b])).to(DEV)
    eager = enc.encode_batch(x)                          # uploads this geometry's descriptors
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # five kernels, a plain linear chain
        res = enc.launch(x)
    graph.replay()
    assert enc.fetch(res) == eager
    pair = (R.make_image(40, 64, "flat"), a)
    x.copy_(torch.from_numpy(np.stack(pair)).to(DEV))
    graph.replay()
    for f, im in zip(enc.fetch(res), pair):
        _assert_same(f, L.encode(im), "graph replay")


def test_round_trip_through_the_device_decoder(single):
    """The decoder's match path on device-written files, not only on zlib's."""
    from wu.png import GPUPngDecoder
    dec = GPUPngDecoder(DEV)
    out, sizes, status = dec.decode_batch([single[n] for n in C.NAMES], return_status=True)
    dec.close()
    assert status == ["ok"] * len(C.NAMES) and dec.stats["native"] == len(C.NAMES) and dec.stats["fallback"] == 0
    out = out.cpu().numpy()
    for i, n in enumerate(C.NAMES):
        img = C.computed(n)[0]
        assert tuple(sizes[i]) == img.shape[:2]
        assert np.array_equal(out[i, :img.shape[0], :img.shape[1]], img), n


def test_matching_none_is_the_encoder_as_it_was():
    from wu.png_enc import GPUPngEncoder
    e = GPUPngEncoder(DEV, matching="none")
    for name in ("16x16_flat", "grid_3x3_of_24", "99x110_gradient_noise"):
        img, _, lit = C.computed(name)
        _assert_same(e.encode_batch(torch.from_numpy(img[None]).to(DEV))[0], lit, f"{name}, matching=none")
    e.close()
    assert e.stats["lz77"] == 0 and e.stats["literal"] + e.stats["stored"] == 4


def test_save_grid_through_the_lz77_encoder_is_smaller(tmp_path, enc):
    from wu.grid import compose_grid
    from wu.infer_driver import save_grid
    from wu.png_enc import GPUPngEncoder
    cells = np.stack([R.make_image(24, 24, "gradient_noise", seed=s) for s in (0, 1, 0, 2, 3, 2)])
    x = (torch.from_numpy(cells).permute(0, 3, 1, 2).float() / 255).to(DEV)
    want = compose_grid(x, 3, 2, False, None, False, 0.0, out="uint8").cpu().numpy()
    plain = GPUPngEncoder(DEV)
    a = save_grid(x, str(tmp_path / "lz.png"), nrow=3, png_encoder=enc)
    b = save_grid(x, str(tmp_path / "none.png"), nrow=3, png_encoder=plain)
    plain.close()
    with open(a, "rb") as fh:
        lz = fh.read()
    with open(b, "rb") as fh:
        none = fh.read()
    assert np.array_equal(_decode(lz), want) and np.array_equal(_decode(none), want)
    assert none == R.encode(want) and lz == L.encode(want)
    assert len(lz) < len(none)
