"""GPU: the quality options of the GIF encoder (wu/gif_enc.py, csrc/gif_enc.hip wu_gif_enc_encode_ex): exact palettes, nearest-colour mapping,
ordered dither, one palette for the animation.  Every file equals the CPU restatement (tests/_gif_quality_ref.py, itself held to its
specification by tests/test_gif_quality_cpu.py) byte for byte, for every case under every option set; no tolerance anywhere."""
import numpy as np
import pytest
import torch

import _gif_enc_ref as R
import _gif_quality_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(C.CASES)
OPTIONS = list(C.OPTIONS)


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def _assert_same(got, want, what):
    assert got == want, f"{what}: {len(got)} bytes vs the restatement's {len(want)}, first difference at byte {_first_diff(got, want)}"


def _device_frames(name):
    """The case's frames on the GPU with the strides the case gives them (a view is taken on the device)."""
    c = C.CASES[name]
    base = torch.from_numpy(c.base).to(DEV)
    return base if c.view is None else base[c.view]


@pytest.fixture(scope="module")
def encoders():
    from wu.gif_enc import GPUGifEncoder
    encs = {o: GPUGifEncoder(DEV, **kw) for o, kw in C.OPTIONS.items()}
    encs["default"] = GPUGifEncoder(DEV)
    yield encs
    for e in encs.values():
        e.close()


@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_files_and_info_equal_the_restatement(encoders, name, options):
    c = C.CASES[name]
    want, info = C.expected(name, options)
    x = _device_frames(name)
    if c.view is not None:
        assert not x.is_contiguous()
    enc = encoders[options]
    res = enc.launch(x)
    got = enc.fetch(res, c.duration_ms, c.loop, c.order)
    got_info = res.info.cpu().numpy()
    assert got_info.shape == (x.shape[0], 2)
    assert got_info.tolist() == [[f["entries"], int(f["exact"])] for f in info], f"{name} / {options}: entries in use, exact path"
    if res.palette is not None:
        assert np.array_equal(res.palette.cpu().numpy().reshape(256, 3), info[0]["palette"]), f"{name} / {options}: global palette"
    _assert_same(got, want, f"{name} / {options}")


def test_best_is_every_option():
    from wu.gif_enc import GPUGifEncoder
    enc = GPUGifEncoder.best(DEV)
    for name in ("grey", "ragged_96x131", "still_left_half_t3"):
        c = C.CASES[name]
        _assert_same(enc.encode(_device_frames(name), c.duration_ms, c.loop, c.order), C.expected(name, "best")[0], name)
    enc.close()


def test_two_runs_give_the_same_bytes(encoders):
    """The histogram, the colour set and its counters are zeroed in-stream: a second launch starts from nothing, whatever ran in between."""
    for options in OPTIONS:
        enc = encoders[options]
        x = _device_frames("ramp_half_noise")
        a, b = enc.launch(x), enc.launch(x)
        fa, fb = enc.fetch(a, 100), enc.fetch(b, 100)
        assert fa == fb
        _assert_same(fa, C.expected("ramp_half_noise", options)[0], f"ramp_half_noise / {options}")
        c = C.CASES["set_collisions_256"]
        _assert_same(enc.encode(_device_frames("set_collisions_256"), c.duration_ms), C.expected("set_collisions_256", options)[0],
                     f"set_collisions_256 / {options}")
        _assert_same(enc.encode(x, 100), C.expected("ramp_half_noise", options)[0], f"ramp_half_noise again / {options}")


def test_launch_in_a_captured_graph_replays_over_new_pixels(encoders):
    """One capture, replayed over a frame that takes the exact path and over one that takes the median cut."""
    enc = encoders["best"]
    names = ["colours_256", "colours_257"]
    x = _device_frames(names[0]).clone()
    eager = enc.encode(x, 100)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # a memset and five kernels, a plain linear chain
        res = enc.launch(x)
    graph.replay()
    assert enc.fetch(res, 100) == eager
    _assert_same(eager, C.expected(names[0], "best")[0], names[0])
    assert res.info.cpu().numpy().tolist() == [[256, 1]]
    x.copy_(_device_frames(names[1]))
    graph.replay()
    _assert_same(enc.fetch(res, 100), C.expected(names[1], "best")[0], "graph replay")
    assert res.info.cpu().numpy()[0, 1] == 0


def test_defaults_are_still_the_first_encoder(encoders):
    for name in NAMES:
        c = C.CASES[name]
        got = encoders["default"].encode(_device_frames(name), c.duration_ms, c.loop, c.order)
        _assert_same(got, R.encode(C.frames(name), c.duration_ms, c.loop, c.order), f"{name} / defaults")


def test_no_flags_through_the_extended_entry_point_are_the_first_encoder_too():
    """wu_gif_enc_encode_ex with flags == 0 runs the kernels of the options over the default rules: the same blocks, and the info."""
    from wu import _lib
    from wu.layout import stream_ptr
    lib = _lib.load()
    for name in ("ragged_96x131", "strided_view", "colours_256"):
        x = _device_frames(name)
        t, h, w = x.shape[:3]
        stride = int(lib.wu_gif_enc_block_stride_ex(h, w, 0))
        ws = torch.empty(int(lib.wu_gif_enc_workspace_bytes_ex(t, h, w, 0)), dtype=torch.uint8, device=DEV)
        out = torch.zeros(t * stride, dtype=torch.uint8, device=DEV)
        result = torch.zeros(t, dtype=torch.int32, device=DEV)
        info = torch.zeros((t, 2), dtype=torch.int32, device=DEV)
        _lib.call("wu_gif_enc_encode_ex", x.data_ptr(), *x.stride(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), result.data_ptr(),
                  t, h, w, 7, 0, None, info.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        want = [R.image_block(f, 7) for f in C.frames(name)]
        for i, (blk, winfo) in enumerate(want):
            n = int(result[i])
            _assert_same(bytes(out[i * stride:i * stride + n].cpu().numpy()), blk, f"{name} frame {i}, flags 0")
            assert info[i].tolist() == [winfo["boxes"], 0]


def test_save_demo_with_the_best_encoder(tmp_path, encoders):
    from wu import infer_driver as D
    frames = _device_frames("still_left_half_t3")
    out = D.save_demo(frames, tmp_path / "demo.gif", gif_encoder=encoders["best"])
    with open(out, "rb") as fh:
        data = fh.read()
    import _gif_quality_ref as Q
    _assert_same(data, Q.encode(C.frames("still_left_half_t3"), 1000 // 3, 0, R.ping_pong(3), **C.OPTIONS["best"]), "save_demo")
