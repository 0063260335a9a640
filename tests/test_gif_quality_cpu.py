"""CPU: the specification of the GIF encoder's quality options and their host half.  tests/_gif_quality_ref.py restates exact palettes,
nearest-colour mapping, ordered dither and the global palette of csrc/gif_enc.hip; here that restatement is held against what it must satisfy
whatever the kernels do: Pillow decodes its files to palette[index], the exact path reproduces small palettes bit for bit, nearest mapping
never loses to box mapping, the dither wins where it should (a smooth ramp, seen through a low-pass) and a still cell stays still under a
global palette.  PSNR figures are printed; only orderings are asserted."""
import ctypes
import io

import numpy as np
import pytest

import _gif_enc_ref as R
import _gif_quality_cases as C
import _gif_quality_ref as Q

NAMES = list(C.CASES)
OPTIONS = list(C.OPTIONS)


def _pillow_frames(data):
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    return im, [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)]


def _decoded(name, options):
    return np.stack([f["palette"][f["index"]] for f in C.expected(name, options)[1]])


@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_decodes_in_pillow_to_palette_of_index(name, options):
    case = C.CASES[name]
    src = C.frames(name)
    data, info = C.expected(name, options)
    order = list(range(len(info))) if case.order is None else case.order
    im, got = _pillow_frames(data)
    assert im.format == "GIF" and im.size == (src.shape[2], src.shape[1])
    assert getattr(im, "n_frames", 1) == len(order) == len(got)
    assert im.info["duration"] == case.duration_ms // 10 * 10 and im.info["loop"] == case.loop
    for g, i in zip(got, order):
        assert np.array_equal(g, info[i]["palette"][info[i]["index"]]), f"{name} / {options}: a frame of source {i} is not palette[index]"
    head = 13 + 19 + (768 if Q.flags_of(**C.OPTIONS[options]) & Q.GLOBAL else 0)
    assert len(data) <= head + len(order) * Q.block_stride(src.shape[1], src.shape[2], Q.flags_of(**C.OPTIONS[options])) + 1
    for f in info:
        assert not f["palette"][f["entries"]:].any() and f["index"].max() < f["entries"]


@pytest.mark.parametrize("name", NAMES)
def test_global_palette_file_decodes_like_local_tables_of_the_same_indices(name):
    """The global colour table changes where the palette is written, not what is shown: the same palette and indices written with a local
    table per frame (the framing of _gif_enc_ref) decode to the same pixels."""
    case = C.CASES[name]
    for options in ("global", "best"):
        data, info = C.expected(name, options)
        assert data[10] == 0xF7 and data[13:13 + 768] == info[0]["palette"].tobytes()
        assert all(np.array_equal(f["palette"], info[0]["palette"]) and f["entries"] == info[0]["entries"] for f in info)
        order = list(range(len(info))) if case.order is None else case.order
        blocks = [Q.image_block(f["palette"], f["index"], case.duration_ms // 10, True)[0] for f in info]
        local = R.header(*C.frames(name).shape[1:3], case.loop) + b"".join(blocks[i] for i in order) + b"\x3B"
        assert len(data) == len(local) + 768 - 768 * len(order)
        for a, b in zip(_pillow_frames(data)[1], _pillow_frames(local)[1]):
            assert np.array_equal(a, b)


def test_exact_reproduces_256_colours_bit_for_bit():
    """What the default mapping cannot do: the grey fixture has 256 colours in 32 bins and comes out at about 41 dB by its bins' boxes."""
    for name in ("grey", "colours_256", "set_collisions_256", "one_pixel", "one_colour"):
        src = C.frames(name)
        for options in ("exact", "best"):
            data, info = C.expected(name, options)
            assert all(f["exact"] for f in info) and info[0]["entries"] == C.distinct(src)
            keys = Q.colour_keys(info[0]["palette"][:info[0]["entries"]])
            assert np.all(np.diff(keys) > 0)                                # ascending r << 16 | g << 8 | b
            got = _pillow_frames(data)[1]
            assert len(got) == len(src) and all(np.array_equal(g, s) for g, s in zip(got, src)), f"{name} / {options}"
    assert not np.array_equal(_decoded("grey", "default")[0], C.frames("grey")[0])


def test_257_colours_take_the_median_cut():
    for name in ("colours_257", "set_collisions_257"):
        for options in ("exact", "best"):
            info = C.expected(name, options)[1]
            assert not info[0]["exact"] and info[0]["entries"] <= 256
    a, b = C.expected("colours_257", "exact"), C.expected("colours_257", "default")
    assert a[0] == b[0]                                                     # exact alone changes nothing above 256 colours


def test_exact_does_not_depend_on_the_order_of_the_pixels():
    src = C.frames("colours_256")[0]
    pal = C.expected("colours_256", "exact")[1][0]["palette"]
    for seed in range(3):
        shuffled = np.random.default_rng(seed).permutation(src.reshape(-1, 3)).reshape(src.shape)
        assert np.array_equal(Q.encode(shuffled[None], 100, exact=True, stats=True)[1][0]["palette"], pal)


@pytest.mark.parametrize("name", NAMES)
def test_nearest_is_never_worse_than_the_box_of_the_bin(name):
    """By construction: both use the same palette, and the nearest entry minimises every pixel's error."""
    src = C.frames(name)
    box, near = R.psnr(_decoded(name, "default"), src), R.psnr(_decoded(name, "nearest"), src)
    print(f"{name}: box {box:.2f} dB, nearest {near:.2f} dB")
    assert near >= box
    a, b = C.expected(name, "default")[1], C.expected(name, "nearest")[1]
    assert all(np.array_equal(x["palette"], y["palette"]) for x, y in zip(a, b))


def test_dither_wins_on_the_ramp_seen_through_a_low_pass():
    src = C.frames("ramp")[0]
    plain = {o: R.psnr(_decoded("ramp", o)[0], src) for o in ("default", "nearest", "nearest_ordered")}
    low = {o: Q.psnr_lowpassed(_decoded("ramp", o)[0], src) for o in ("default", "nearest", "nearest_ordered")}
    print("ramp, plain PSNR:", plain, "low-passed:", low)
    assert low["nearest_ordered"] > low["nearest"] > low["default"]
    src = C.frames("ramp_half_noise")[0]
    low = {o: Q.psnr_lowpassed(_decoded("ramp_half_noise", o)[0], src) for o in ("default", "nearest", "nearest_ordered")}
    print("ramp, lower half noise, low-passed:", low)
    assert low["nearest_ordered"] >= low["nearest"]
    sizes = {o: len(C.expected("ramp", o)[0]) for o in ("default", "nearest", "nearest_ordered")}
    print("ramp, file bytes:", sizes)                                       # the dithered index stream compresses less well


def test_threshold_matrix_and_offsets():
    m = Q.threshold(*np.meshgrid(np.arange(8), np.arange(8), indexing="xy"))
    assert sorted(m.reshape(-1).tolist()) == list(range(64)) and m[0, 0] == 0
    assert m[0, 1] == 32 and m[1, 0] == 48 and m[1, 1] == 16               # [y, x]: bit 0 of x and y carries the highest digit
    assert np.array_equal(Q.threshold(np.arange(8) + 8, np.arange(8) + 16), Q.threshold(np.arange(8), np.arange(8)))
    off = ((2 * m + 1 - 64) * 16) // 128
    assert off.min() == -8 and off.max() == 7 and abs(int(off.sum())) <= 32  # one step of 16, centred


def test_ties_go_to_the_lowest_index():
    info = C.expected("ties", "nearest")[1][0]
    src = C.frames("ties")[0].reshape(-1, 3).astype(np.int64)
    pal = info["palette"][:info["entries"]].astype(np.int64)
    d = ((src[:, None] - pal[None]) ** 2).sum(2)
    tied = (d == d.min(1, keepdims=True)).sum(1) > 1
    assert tied.sum() >= 12
    first = np.argmax(d == d.min(1, keepdims=True), 1)
    assert np.array_equal(info["index"].reshape(-1), first)


def test_the_still_half_stays_still_under_a_global_palette():
    src = C.frames("still_left_half_t3")
    for options in ("global", "best"):
        dec = _pillow_frames(C.expected("still_left_half_t3", options)[0])[1]
        assert len(dec) == 4
        assert all(np.array_equal(d[:, :24], dec[0][:, :24]) for d in dec), options
    for kw in (dict(mapping="nearest", palette="global"), dict(mapping="nearest", dither="ordered", palette="global")):
        info = Q.encode(src, 250, stats=True, **kw)[1]
        assert all(np.array_equal(f["index"][:, :24], info[0]["index"][:, :24]) for f in info)
    local = _decoded("still_left_half_t3", "default")
    assert not np.array_equal(local[0][:, :24], local[1][:, :24])           # what a palette per frame does to the same cell


def test_defaults_are_the_first_encoder_byte_for_byte():
    for name in NAMES:
        c = C.CASES[name]
        assert C.expected(name, "default")[0] == R.encode(C.frames(name), c.duration_ms, c.loop, c.order), name
    assert Q.flags_of() == 0 and Q.block_stride(37, 53) == R.block_stride(37, 53) == Q.block_stride(37, 53, Q.GLOBAL) + 768


def test_argument_errors():
    from wu.gif_enc import GPUGifEncoder, option_flags
    for kw in (dict(mapping="closest"), dict(dither="floyd"), dict(dither=True), dict(palette="shared"), dict(exact=1), dict(exact="yes"),
               dict(dither="ordered"), dict(dither="ordered", mapping="box")):
        with pytest.raises(ValueError):
            GPUGifEncoder(**kw)
        with pytest.raises(ValueError):
            Q.flags_of(**kw)
    for name, kw in C.OPTIONS.items():
        assert option_flags(**kw) == Q.flags_of(**kw) == GPUGifEncoder(**kw).flags
    assert GPUGifEncoder().flags == 0 and GPUGifEncoder.best().flags == 15 == Q.flags_of(**C.OPTIONS["best"])
    best = GPUGifEncoder.best()
    assert (best.mapping, best.dither, best.exact, best.palette) == ("nearest", "ordered", True, "global")


def test_abi_agrees_with_the_restatement_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    for h, w in [C.frames(n).shape[1:3] for n in NAMES] + [(224, 224), (1576, 3868), (1, 65535), (8192, 8192)]:
        for flags in (0, 1, 3, 4, 8, 15):
            assert lib.wu_gif_enc_block_stride_ex(h, w, flags) == Q.block_stride(h, w, flags) > 0, (h, w, flags)
        assert lib.wu_gif_enc_block_stride_ex(h, w, 0) == lib.wu_gif_enc_block_stride(h, w)
        assert 0 < lib.wu_gif_enc_workspace_bytes_ex(2, h, w, 0) - lib.wu_gif_enc_workspace_bytes(2, h, w) <= 256       # the palettes' info
    for flags in (2, 6, 10, 16, -1):                                        # dither without nearest; unknown bits
        assert lib.wu_gif_enc_block_stride_ex(8, 8, flags) == 0 == lib.wu_gif_enc_workspace_bytes_ex(1, 8, 8, flags)
    assert lib.wu_gif_enc_workspace_bytes_ex(3, 128, 130, 8) < lib.wu_gif_enc_workspace_bytes_ex(3, 128, 130, 0)     # one histogram
    assert lib.wu_gif_enc_workspace_bytes_ex(3, 128, 130, 4) > lib.wu_gif_enc_workspace_bytes_ex(3, 128, 130, 0)     # the colour sets
    assert lib.wu_gif_enc_workspace_bytes_ex(64, 8192, 8192, 0) > 0
    assert lib.wu_gif_enc_workspace_bytes_ex(63, 8192, 8192, 8) > 0 and lib.wu_gif_enc_workspace_bytes_ex(64, 8192, 8192, 8) == 0   # 2^32 pixels
    one = ctypes.c_void_p(256)           # a non-null, aligned pointer that is never dereferenced: every call below fails validation first
    args = dict(frames=one, st=192, sy=24, sx=3, sc=1, ws=one, ws_bytes=1 << 30, out=one, out_bytes=1 << 30, result=one, T=1, H=8, W=8,
                delay=10, flags=15, palette=one, info=one, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.wu_gif_enc_encode_ex(*a.values())
    assert call(info=None) < 0 and b"null" in lib.wu_last_error()
    assert call(flags=2) < 0 and b"bad flags" in lib.wu_last_error()
    assert call(flags=16) < 0 and b"bad flags" in lib.wu_last_error()
    assert call(palette=None) < 0 and b"palette_dev" in lib.wu_last_error()
    assert call(T=0) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(sy=-24) < 0 and b"negative" in lib.wu_last_error()
    assert call(delay=65536) < 0 and b"delay" in lib.wu_last_error()
    assert call(ws_bytes=16) < 0 and b"workspace too small" in lib.wu_last_error()
    assert call(out_bytes=16) < 0 and b"output too small" in lib.wu_last_error()
    assert call(info=ctypes.c_void_p(258)) < 0 and b"aligned" in lib.wu_last_error()


def test_encoder_with_options_refuses_cpu_tensors():
    import torch
    from wu.gif_enc import GPUGifEncoder
    enc = GPUGifEncoder.best()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 100)
    enc.close()
