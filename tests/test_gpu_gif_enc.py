"""GPU: the GIF encoder (wu/gif_enc.py, csrc/gif_enc.hip).  A GIF is a palette image and Pillow orders its palette differently, so Pillow's
bytes are not the bar.  The bar: every file equals the CPU restatement (tests/_gif_enc_ref.py, itself validated by tests/test_gif_enc_cpu.py)
byte for byte, and Pillow decodes it to palette[index]; no tolerance anywhere."""
import io

import numpy as np
import pytest
import torch

import _gif_enc_cases as C
import _gif_enc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(C.CASES)


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
def enc():
    from wu.gif_enc import GPUGifEncoder
    e = GPUGifEncoder(DEV)
    yield e
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_files_equal_the_restatement_and_decode(enc, name):
    from PIL import Image, ImageSequence
    c = C.CASES[name]
    want, info = C.expected(name)
    x = _device_frames(name)
    if c.view is not None:
        assert not x.is_contiguous()
    before = enc.stats["frames"]
    got = enc.encode(x, c.duration_ms, c.loop, c.order)
    assert enc.stats["frames"] == before + x.shape[0]
    _assert_same(got, want, name)
    order = list(range(len(info))) if c.order is None else c.order
    frames = [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(got)))]
    assert len(frames) == len(order)
    for f, i in zip(frames, order):
        assert np.array_equal(f, info[i]["palette"][info[i]["index"]])
    assert len(got) <= 32 + len(order) * R.block_stride(x.shape[1], x.shape[2]) + 1


def test_cases_of_equal_geometry_in_one_launch_are_independent(enc):
    """All cases of one frame size go through ONE launch; every case's file is then assembled from its own frames' blocks."""
    groups = {}
    for name in NAMES:
        groups.setdefault(tuple(C.frames(name).shape[1:3]), []).append(name)
    shared = {k: v for k, v in groups.items() if len(v) > 1}
    assert (72, 128) in shared and len(shared[(72, 128)]) == 4 and (9, 11) in shared
    for names in shared.values():
        stack = torch.cat([_device_frames(n).contiguous() for n in names])
        res = enc.launch(stack)
        at = 0
        for n in names:
            c = C.CASES[n]
            t = C.frames(n).shape[0]
            order = range(t) if c.order is None else c.order
            got = enc.fetch(res, c.duration_ms, c.loop, [at + i for i in order])
            _assert_same(got, C.expected(n)[0], f"{n} in a batch of {stack.shape[0]} frames")
            at += t


def test_two_launches_give_identical_bytes(enc):
    """The workspace is zeroed in-stream: a second launch does not add to the first one's histogram."""
    x = _device_frames("noise")
    a, b = enc.launch(x), enc.launch(x)
    fa, fb = enc.fetch(a, 70), enc.fetch(b, 70)
    assert fa == fb
    _assert_same(fa, C.expected("noise")[0], "noise")
    y = _device_frames("flat")                                       # ... nor does a launch of another geometry in between
    _assert_same(enc.encode(y, 100), C.expected("flat")[0], "flat")
    _assert_same(enc.encode(x, 70), C.expected("noise")[0], "noise again")


def test_launch_in_a_captured_graph_replays_over_new_pixels(enc):
    names = ["width_edge_a645", "width_edge_a1000"]
    x = _device_frames(names[0]).clone()
    eager = enc.encode(x, 100)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # a memset and five kernels, a plain linear chain
        res = enc.launch(x)
    graph.replay()
    assert enc.fetch(res, 100) == eager
    _assert_same(eager, C.expected(names[0])[0], names[0])
    x.copy_(_device_frames(names[1]))
    graph.replay()
    _assert_same(enc.fetch(res, 100), C.expected(names[1])[0], "graph replay")


def test_save_demo_with_the_encoder(tmp_path, enc):
    from PIL import Image
    from wu import grid, infer_driver as D
    g = torch.Generator().manual_seed(7)
    B, nc, T, h, w = 2, 2, 3, 8, 8
    batch = torch.rand(B, 3, h, w, generator=g)
    results = torch.rand(T, nc, B, 3, h, w, generator=g)
    frames = grid.demo_tables(batch.to(DEV), results.to(DEV))
    assert frames.dtype == torch.uint8 and frames.shape[0] == T and frames.shape[3] == 3
    out = D.save_demo(frames, tmp_path / "demo.gif", gif_encoder=enc)
    with open(out, "rb") as fh:
        data = fh.read()
    _assert_same(data, R.encode(frames.cpu().numpy(), 1000 // T, 0, R.ping_pong(T)), "save_demo")
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == 2 * T - 2 and im.size == (frames.shape[2], frames.shape[1])
    assert im.info.get("loop") == 0 and im.info.get("duration") == (1000 // T) // 10 * 10
    with pytest.raises(ValueError):
        enc.fetch(enc.launch(frames), 100, 0, [0, T])
