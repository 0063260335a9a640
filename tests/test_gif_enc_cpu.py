"""CPU: the GIF encoder's specification and its host half.  tests/_gif_enc_ref.py restates csrc/gif_enc.hip; here that restatement is
itself held against what it must satisfy whatever the kernels do -- Pillow opens its files with the right frame count, duration and loop
and decodes every frame to palette[index], the cases built to be exact are exact, no file exceeds the worst-case bound, and the quantiser
is no worse than Pillow's own adaptive palette.  tests/_gif_enc_cases.py asserts at import that every case reaches the edge it is named for."""
import ctypes
import io

import numpy as np
import pytest

import _gif_enc_cases as C
import _gif_enc_ref as R

NAMES = list(C.CASES)


def _pillow_frames(data):
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    frames = [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)]
    return im, frames


@pytest.mark.parametrize("name", NAMES)
def test_restatement_decodes_in_pillow_to_palette_of_index(name):
    case = C.CASES[name]
    src = C.frames(name)
    data, info = C.expected(name)
    order = list(range(len(info))) if case.order is None else case.order
    im, got = _pillow_frames(data)
    assert im.format == "GIF" and im.size == (src.shape[2], src.shape[1])
    assert getattr(im, "n_frames", 1) == len(order) == len(got)
    assert im.info["duration"] == case.duration_ms // 10 * 10
    if case.loop is None:
        assert "loop" not in im.info
    else:
        assert im.info["loop"] == case.loop
    for g, i in zip(got, order):
        assert np.array_equal(g, info[i]["palette"][info[i]["index"]]), f"{name}: a frame of source {i} is not palette[index]"
        if case.lossless:
            assert np.array_equal(g, src[i]), f"{name}: frame {i} is not the input"


@pytest.mark.parametrize("name", NAMES)
def test_size_is_bounded_by_the_block_stride(name):
    case = C.CASES[name]
    src = C.frames(name)
    data, info = C.expected(name)
    order = list(range(len(info))) if case.order is None else case.order
    head = 13 + (0 if case.loop is None else 19)
    assert len(data) <= head + len(order) * R.block_stride(src.shape[1], src.shape[2]) + 1
    for f in info:
        assert f["payload"] == (sum(s["bits"] for s in f["segments"]) + 7) // 8
        assert all(18 <= s["bits"] <= 12 * (R.SEGMENT + 4) for s in f["segments"])


def test_every_distinct_frame_is_coded_once_and_repeats_reuse_its_block():
    src = C.frames("few_colours")
    blocks = [R.image_block(f, 33)[0] for f in src]
    data = C.expected("few_colours")[0]
    assert C.CASES["few_colours"].order == [0, 1, 2, 1]
    assert data == R.header(37, 53, 0) + blocks[0] + blocks[1] + blocks[2] + blocks[1] + b"\x3B"


def test_trailing_code_at_the_unbumped_width_is_a_broken_stream():
    """The width rule at segment ends is load-bearing: the same segments with the trailing Clear one bit short do not decode."""
    index = R.quantise(C.frames("width_edge_a128")[0])[1].reshape(-1)
    acc, nbits, st = R.lzw_segment(index[:R.SEGMENT], True, False)
    assert st["bump"] and st["width"] == 10
    short = acc & ((1 << (nbits - 10)) - 1) | (R.CLEAR << (nbits - 10))           # the Clear at 9 bits
    a2, n2, _ = R.lzw_segment(index[R.SEGMENT:], False, True)
    payload = (short | (a2 << (nbits - 1))).to_bytes((nbits - 1 + n2 + 7) // 8, "little")
    good, _ = R.image_block(C.frames("width_edge_a128")[0], 10)
    bad = bytearray(good[:R.BLOCK_FIXED])
    for at in range(0, len(payload), 255):
        bad += bytes([len(payload[at:at + 255])]) + payload[at:at + 255]
    bad += b"\x00"
    from PIL import Image
    ok = np.asarray(Image.open(io.BytesIO(R.header(72, 128, 0) + good + b"\x3B")).convert("RGB"))
    assert np.array_equal(ok, C.frames("width_edge_a128")[0])
    try:
        broken = np.asarray(Image.open(io.BytesIO(R.header(72, 128, 0) + bytes(bad) + b"\x3B")).convert("RGB"))
    except (OSError, EOFError, ValueError):
        return
    assert not np.array_equal(broken, ok)


@pytest.mark.parametrize("name", ["natural", "noise"])
def test_quantiser_is_no_worse_than_pillows_adaptive_palette(name):
    from PIL import Image
    for src, f in zip(C.frames(name), C.expected(name)[1]):
        ours = R.psnr(f["palette"][f["index"]], src)
        pil = R.psnr(np.asarray(Image.fromarray(src).convert("P", palette=Image.ADAPTIVE).convert("RGB")), src)
        print(f"{name}: restatement {ours:.2f} dB, Pillow ADAPTIVE {pil:.2f} dB")
        assert ours >= pil


def test_several_colours_in_one_bin_are_not_told_apart():
    """The documented limitation: 256 greys are 32 bins, so 32 palette entries."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2).repeat(4, axis=0)
    pal, idx, boxes = R.quantise(ramp)
    assert boxes == 32 and not np.array_equal(pal[idx], ramp) and 38.0 < R.psnr(pal[idx], ramp) < 44.0


def test_abi_agrees_with_the_restatement_without_a_gpu():
    from wu import _lib, gif_enc
    lib = _lib.load()
    assert lib.wu_gif_enc_segment_pixels() == R.SEGMENT == 8192 == gif_enc.segment_pixels()
    sizes = [C.frames(n).shape[1:3] for n in NAMES] + [(224, 224), (1576, 3868), (1, 65535), (65535, 1), (8192, 8192), (1024, 65535)]
    for h, w in sizes:
        assert lib.wu_gif_enc_block_stride(h, w) == R.block_stride(h, w) == gif_enc.block_stride(h, w) > 0, (h, w)
    for h, w in ((0, 8), (8, 0), (65536, 1), (1, 65536), (8193, 8192), (65535, 65535)):
        assert lib.wu_gif_enc_block_stride(h, w) == 0 == R.block_stride(h, w), (h, w)
        assert lib.wu_gif_enc_workspace_bytes(1, h, w) == 0
        with pytest.raises(ValueError):
            gif_enc.block_stride(h, w)
    base = lib.wu_gif_enc_workspace_bytes(2, 128, 130)
    assert base >= 2 * (32768 * 28 + 3 * 12 * (8192 + 4) // 8)            # the histogram and one slot per segment, at least
    assert lib.wu_gif_enc_workspace_bytes(4, 128, 130) > base and lib.wu_gif_enc_workspace_bytes(2, 300, 130) > base
    assert lib.wu_gif_enc_workspace_bytes(0, 8, 8) == 0 and lib.wu_gif_enc_workspace_bytes(65536, 8, 8) == 0
    assert gif_enc.ping_pong(1) == [0] and gif_enc.ping_pong(2) == [0, 1] and gif_enc.ping_pong(4) == [0, 1, 2, 3, 2, 1] == R.ping_pong(4)
    # the entry point validates before it launches anything
    one = ctypes.c_void_p(256)           # a non-null, aligned pointer that is never dereferenced: every call below fails validation first
    args = dict(frames=one, st=192, sy=24, sx=3, sc=1, ws=one, ws_bytes=1 << 30, out=one, out_bytes=1 << 30, result=one, T=1, H=8, W=8,
                delay=10, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.wu_gif_enc_encode(*a.values())
    assert call(frames=None) < 0 and b"null" in lib.wu_last_error()
    assert call(T=0) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(W=70000) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(H=8193, W=8192) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(sy=-24) < 0 and b"negative" in lib.wu_last_error()
    assert call(delay=65536) < 0 and b"delay" in lib.wu_last_error()
    assert call(ws_bytes=16) < 0 and b"workspace too small" in lib.wu_last_error()
    assert call(out_bytes=16) < 0 and b"output too small" in lib.wu_last_error()
    assert call(ws=ctypes.c_void_p(257)) < 0 and b"aligned" in lib.wu_last_error()


def test_encoder_refuses_cpu_tensors_and_bad_frames():
    import torch
    from wu.gif_enc import GPUGifEncoder
    enc = GPUGifEncoder(device="cuda")                   # constructing needs no GPU
    assert enc.segment_pixels == R.SEGMENT and enc.stats == {"frames": 0, "bytes": 0}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.launch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 100)
    with pytest.raises(ValueError):
        enc.launch(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        enc.launch(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        enc.launch(np.zeros((1, 8, 8, 3), np.uint8))
    enc.close()


def test_save_demo_keeps_the_gif_on_pillow_without_an_encoder(tmp_path):
    """gif_encoder=None changes nothing: the default, and the file Pillow writes -- one global colour table, no local ones."""
    import inspect
    import torch
    from PIL import Image
    from wu import infer_driver as D
    assert inspect.signature(D.save_demo).parameters["gif_encoder"].default is None
    rgb = C.frames("ping_pong_t3")
    out = D.save_demo(torch.from_numpy(np.ascontiguousarray(rgb)), tmp_path / "demo.gif")
    with open(out, "rb") as fh:
        data = fh.read()
    imgs = [Image.fromarray(f).convert("RGB") for f in rgb]
    buf = io.BytesIO()
    imgs[0].save(buf, "GIF", save_all=True, append_images=imgs[1:] + imgs[1:-1][::-1], duration=1000 // 3, loop=0)
    assert data == buf.getvalue()
    assert data[10] & 0x80 and data != C.expected("ping_pong_t3")[0]                   # Pillow's: a global colour table; ours has none (0x70)
    assert C.expected("ping_pong_t3")[0][10] == 0x70
