"""GPU: image grids and tables (wu/grid.py, csrc/grid.hip) against the CPU restatement of torchvision 0.3's make_grid
(tests/_grid_ref.py, itself pinned by tests/test_grid_cpu.py).  Every operation of the kernels is a specified, correctly rounded fp32
operation, so equality is exact everywhere: torch.equal on fp32 bits and on bytes, no tolerance."""
import io
import os

import numpy as np
import pytest
import torch

import _grid_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rand(*shape, seed=0, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _check_grid(x_dev, ref_in=None, **kw):
    """make_grid on the GPU, both output kinds, against the restatement on the CPU copy."""
    from wu import grid
    if ref_in is None:
        ref_in = [t.cpu() for t in x_dev] if isinstance(x_dev, list) else x_dev.cpu()
    want = R.make_grid(ref_in, **kw)
    got = grid.make_grid(x_dev, **kw)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), kw
    got8 = grid.compose_grid(x_dev, out="uint8", **kw)
    assert got8.dtype == torch.uint8 and torch.equal(got8.cpu(), R.to_u8(want)), kw
    return want


@pytest.mark.parametrize("normalize,scale_each", [(False, False), (True, False), (True, True)])
def test_ragged_grid_of_odd_images(normalize, scale_each):
    x = _rand(3, 3, 5, 7, seed=1).to(DEV)
    want = _check_grid(x, nrow=2, normalize=normalize, scale_each=scale_each, pad_value=0.5)
    assert want.shape == (3, 16, 20) and torch.all(want[:, 9:14, 11:18] == 0.5)
    _check_grid(x, nrow=2, padding=0, normalize=normalize, scale_each=scale_each)
    _check_grid(x, nrow=8, padding=3, normalize=normalize, scale_each=scale_each, pad_value=1.0)


def test_one_image_is_returned_alone_and_equals_save_images_bytes():
    from wu import grid, infer_driver as D
    x = _rand(1, 3, 5, 7, seed=2).to(DEV)
    want = _check_grid(x, normalize=True, scale_each=True)
    assert want.shape == (3, 5, 7)
    _check_grid(x[0], normalize=True)
    got8 = grid.compose_grid(x, normalize=True, out="uint8")
    assert torch.equal(got8, D.to_uint8(D.normalize_minmax(x))[0])          # the bytes save_images writes today


def test_one_group_spanning_the_batch():
    x = _rand(4, 3, 16, 16, seed=3).to(DEV)
    _check_grid(x, nrow=2, normalize=True, scale_each=False)
    _check_grid(list(x), nrow=3, normalize=True, scale_each=False)             # a list of (3, H, W) images, not stacked


def test_constant_image_and_explicit_range():
    x = _rand(3, 3, 6, 9, seed=4)
    x[1] = 0.75                                                              # hi == lo: exact zeros
    want = _check_grid(x.to(DEV), nrow=3, normalize=True, scale_each=True)
    assert torch.all(want[:, 2:8, 13:22] == 0)
    y = _rand(2, 3, 6, 9, seed=5, scale=2.0)
    assert y.min() < -1 and y.max() > 1                                       # samples outside the range are clamped
    want = _check_grid(y.to(DEV), normalize=True, value_range=(-1.0, 1.0))
    assert want.min() == 0 and want.max() < 1
    from wu import grid
    assert torch.equal(grid.make_grid(y.to(DEV), normalize=True, range=(-1.0, 1.0)).cpu(), want)


def test_element_types_layouts_and_slices():
    x = _rand(3, 3, 10, 13, seed=6)
    for kw in ({"normalize": True, "scale_each": True}, {"normalize": False}):
        xb = x.to(DEV).bfloat16()                                            # bf16 NCHW
        _check_grid(xb, nrow=2, **kw)
        xc = x.to(DEV).contiguous(memory_format=torch.channels_last)         # fp32 channels-last: sx = 3
        assert xc.stride(3) == 3
        _check_grid(xc, nrow=2, **kw)
        big = _rand(5, 6, 20, 30, seed=7).to(DEV)
        _check_grid(big[1:4, 2:5, 3:17, 5:28], nrow=2, **kw)                 # a slice: odd row starts, contiguous rows
        _check_grid(big[1:4, 0:3, 1:20:2, 2:30:3], nrow=3, **kw)             # strided in y and x
        bigb = big.bfloat16()
        _check_grid(bigb[0:2, 1:4, 2:9, 1:24], **kw)
        wide = _rand(2, 3, 4, 300, seed=8).to(DEV)                            # wider than one wave's 256 pixels
        _check_grid(wide, nrow=1, **kw)
        _check_grid(wide.bfloat16()[:, :, :, 1:], nrow=1, **kw)


def test_ranges_cover_the_whole_cell_and_nothing_else():
    from wu import grid
    x = torch.rand(2, 3, 67, 129, generator=torch.Generator().manual_seed(9))
    x[0, 2, 66, 128] = -7.0                                                   # the minimum: last element of image 0
    x[1, 0, 0, 0] = 9.0                                                       # the maximum: first element of image 1
    xd = x.to(DEV)
    comp = grid.composer(xd.device)
    grid.make_grid(xd, normalize=True, scale_each=True)
    got = comp.ranges().cpu()
    want = torch.stack([torch.stack([x[i].min(), x[i].max()]) for i in range(2)])
    assert torch.equal(got, want) and got[0, 0] == -7.0 and got[1, 1] == 9.0
    grid.make_grid(xd, normalize=True, scale_each=False)
    assert torch.equal(comp.ranges().cpu(), torch.tensor([[-7.0, 9.0]]))
    _check_grid(xd, normalize=True, scale_each=True)
    _check_grid(xd.bfloat16(), normalize=True, scale_each=False)


@pytest.fixture(scope="module")
def demo():
    T, nc, B, h, w = 2, 3, 2, 8, 8
    batch, results = _rand(B, 3, h, w, seed=10), _rand(T, nc, B, 3, h, w, seed=11, scale=0.6)
    return batch, results, R.demo_tables(batch, results)


def test_demo_tables_both_kinds_and_frame_by_frame(demo):
    from wu import grid
    batch, results, want = demo
    bd, rd = batch.to(DEV), results.to(DEV)
    assert want.shape == (2, 3, 22, 48)
    got = grid.demo_tables(bd, rd, out="float")
    assert torch.equal(got.cpu(), want)
    got8 = grid.demo_tables(bd, rd)
    assert got8.shape == (2, 22, 48, 3) and torch.equal(got8.cpu(), R.to_u8(want))
    for t in range(2):                                                       # all frames in one call == frame-by-frame calls
        assert torch.equal(grid.demo_tables(bd, rd[t:t + 1])[0], got8[t])
        assert torch.equal(grid.demo_tables(bd, rd[t:t + 1], out="float")[0], got[t])


def test_demo_frames_through_a_real_network():
    import cunet
    from wu import infer_driver as D
    torch.manual_seed(0)
    net = cunet.Conditional_UNet(3).to(DEV).eval()
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
    pred = torch.randn(2, 3, generator=g).to(DEV)
    thetas = (-0.7, 0.9)
    frames = D.demo_frames(net, x, pred, thetas)
    raw = D.axis_sweep(net, x, pred, thetas)
    assert raw.shape == (2, 3, 2, 3, 16, 16)
    want = R.to_u8(R.demo_tables(x.cpu(), raw.cpu()))
    assert frames.dtype == torch.uint8 and frames.shape == (2, 2 * 18 + 2, 4 * 20, 3)
    assert torch.equal(frames.cpu(), want)


def test_summary_image():
    from wu import grid
    from wu.train_step import WeatherTransferStep
    B, h, w = 2, 8, 8
    images, fakes = _rand(B, 3, h, w, seed=13), _rand(B, B, 3, h, w, seed=14)
    ref = _rand(B, 3, h, w, seed=15).abs() + 0.5                              # all positive: strip 0's minimum is the blank's zero
    want = R.summary_image(images, ref, fakes)
    assert want.shape == (3, 32, 28)
    got = WeatherTransferStep.summary_image(images.to(DEV), ref.to(DEV), fakes.to(DEV))
    assert torch.equal(got.cpu(), want)
    rng = grid.composer(torch.device(DEV)).ranges().cpu()
    assert rng[0, 0] == 0 and rng[0, 1] == ref.max()
    got8 = grid.summary_image(images.to(DEV), ref.to(DEV), fakes.to(DEV), out="uint8")
    assert torch.equal(got8.cpu(), R.to_u8(want))


def _decode(path):
    from PIL import Image
    with open(path, "rb") as fh:
        data = fh.read()
    Image.open(io.BytesIO(data)).verify()
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_save_grid_files(tmp_path):
    from PIL import Image
    from wu import infer_driver as D
    from wu.png_enc import GPUPngEncoder
    x = _rand(4, 3, 16, 16, seed=16)
    ref_u8 = R.to_u8(R.make_grid(x, nrow=2, normalize=True, scale_each=True, pad_value=0.25)).numpy()
    kw = dict(nrow=2, normalize=True, scale_each=True, pad_value=0.25)
    xd = x.to(DEV)
    D.save_grid(xd, tmp_path / "pillow.png", **kw)
    assert np.array_equal(_decode(tmp_path / "pillow.png"), ref_u8)
    enc = GPUPngEncoder(DEV)
    try:
        D.save_grid(xd, tmp_path / "gpu.png", png_encoder=enc, **kw)
    finally:
        enc.close()
    assert np.array_equal(_decode(tmp_path / "gpu.png"), ref_u8)
    D.save_grid(xd, tmp_path / "t.jpg", **kw)
    Image.fromarray(ref_u8).save(tmp_path / "ref.jpg")
    assert (tmp_path / "t.jpg").read_bytes() == (tmp_path / "ref.jpg").read_bytes()


def test_save_demo_directory_and_gif(tmp_path, demo):
    from PIL import Image
    from wu import grid, infer_driver as D
    batch, results, want = demo
    results3 = torch.cat([results, results[:1] * 0.5])                       # T = 3: the ping-pong has 2 T - 2 = 4 frames
    frames = grid.demo_tables(batch.to(DEV), results3.to(DEV))
    want8 = R.to_u8(R.demo_tables(batch, results3)).numpy()
    T, hg, wg = 3, 22, 48
    paths = D.save_demo(frames, tmp_path / "jpg")
    assert len(paths) == T and all(p.endswith(".jpg") for p in paths)
    for p in paths:
        assert _decode(p).shape == (hg, wg, 3)
    paths = D.save_demo(frames, tmp_path / "png", ext=".png")
    for t, p in enumerate(paths):
        assert np.array_equal(_decode(p), want8[t])
    gif = D.save_demo(frames, tmp_path / "demo.gif")
    im = Image.open(gif)
    assert im.n_frames == 2 * T - 2 and im.size == (wg, hg)
    assert im.info.get("loop") == 0 and im.info.get("duration") == (1000 // T) // 10 * 10      # GIF delays are centiseconds


def test_compose_in_a_captured_graph_replays_over_new_sources(demo):
    from wu import grid
    batch, results, _ = demo
    bd, rd = batch.to(DEV), results.to(DEV)
    grid.demo_tables(bd, rd)                                                  # uploads the descriptors of (plan, these tensors)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                # three kernels, a plain linear chain
        out8 = grid.demo_tables(bd, rd)
        outf = grid.demo_tables(bd, rd, out="float")
    for seed in (20, 21):
        nb, nr = _rand(*batch.shape, seed=seed), _rand(*results.shape, seed=seed + 5, scale=0.4)
        bd.copy_(nb.to(DEV))
        rd.copy_(nr.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = R.demo_tables(nb, nr)
        assert torch.equal(outf.cpu(), want) and torch.equal(out8.cpu(), R.to_u8(want))


def test_a_plan_never_composed_cannot_be_captured(monkeypatch):
    from wu import grid
    x = _rand(2, 3, 6, 6, seed=30).to(DEV)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="outside the capture"):
        grid.make_grid(x)


def test_three_launches_whatever_the_number_of_cells(demo):
    """Counts the launches wu_grid_compose brackets with wu_prof_pre / wu_prof_post (all it makes); the profiler test below counts
    what the device ran."""
    from wu import _lib, grid
    batch, results, _ = demo
    bd, rd = batch.to(DEV), results.to(DEV)
    x = _rand(9, 3, 6, 6, seed=31).to(DEV)
    grid.demo_tables(bd, rd)
    grid.make_grid(x, normalize=True)
    for fn in (lambda: grid.demo_tables(bd, rd), lambda: grid.make_grid(x, normalize=True), lambda: grid.make_grid(x[:1])):
        _lib.prof_begin([_lib.FAM_GRID], 16)
        try:
            fn()
            n = _lib.prof_query(_lib.FAM_GRID)["launches"]
        finally:
            _lib.prof_end()
        assert 1 <= n <= 3, n


def test_device_kernels_per_compose_counted_by_the_profiler(demo):
    """The count above is of the launches wu_grid_compose brackets itself; this one is of every kernel the device ran during one
    compose, whoever launched it: a torch op slipped into GridComposer.compose would show here."""
    from torch.profiler import ProfilerActivity, profile
    from wu import grid
    batch, results, _ = demo
    bd, rd = batch.to(DEV), results.to(DEV)
    grid.demo_tables(bd, rd)                                                  # descriptors uploaded: no copy inside the window
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        grid.demo_tables(bd, rd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    print("device events of one compose:", names)
    assert 1 <= len(kernels) <= 3 and all("grid_" in n for n in kernels), names


def test_a_captured_graph_outlives_any_number_of_other_bindings(demo):
    """A graph holds the address of the descriptors it was captured with: they are pinned, so more other (plan, sources) pairs than
    the cache keeps do not free them, and the graph's workspace and outputs are its own."""
    from wu import grid
    batch, results, _ = demo
    bd, rd = batch.to(DEV).clone(), results.to(DEV).clone()
    comp = grid.composer(torch.device(DEV))
    grid.demo_tables(bd, rd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out8 = grid.demo_tables(bd, rd)
    pinned = [d for d in comp._desc.values() if d.pinned]
    assert pinned
    others = [_rand(1, 3, 4, 4, seed=100 + i).to(DEV) for i in range(comp.MAX_CACHED + 8)]       # alive together: distinct addresses
    for i, o in enumerate(others):
        got = grid.make_grid(o, normalize=True)
        if i % 16 == 0:
            assert torch.equal(got.cpu(), R.make_grid(o.cpu(), normalize=True))
    assert len(comp._desc) <= comp.MAX_CACHED + len(pinned)                   # the cache stayed bounded ...
    assert all(any(d is p for d in comp._desc.values()) for p in pinned)      # ... and dropped none a graph reads (checked BEFORE the replay)
    junk = [torch.full((2048,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(64)]          # whatever was freed is handed out again
    nb, nr = _rand(*batch.shape, seed=40), _rand(*results.shape, seed=41, scale=0.4)
    bd.copy_(nb.to(DEV))
    rd.copy_(nr.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out8.cpu(), R.to_u8(R.demo_tables(nb, nr)))
    del junk


def test_two_streams_do_not_share_a_workspace():
    from wu import grid
    x = _rand(3, 3, 9, 11, seed=50)
    xd = x.to(DEV)
    comp = grid.composer(xd.device)
    want = R.make_grid(x, nrow=2, normalize=True, scale_each=True)
    grid.make_grid(xd, nrow=2, normalize=True, scale_each=True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    ws, got = [], []
    for s in (s1, s2):
        with torch.cuda.stream(s):
            got.append(grid.make_grid(xd, nrow=2, normalize=True, scale_each=True))
            ws.append(comp.ranges().data_ptr())
    torch.cuda.synchronize()
    assert ws[0] != ws[1]
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want)


def test_sources_are_indexed_inside_their_bounds():
    from wu import grid
    x = _rand(2, 3, 6, 6, seed=51).to(DEV)
    comp = grid.composer(x.device)
    with pytest.raises(IndexError):
        comp.compose(grid.plan_grid(3, 6, 6), x)                              # the plan's third image is not there
    with pytest.raises(ValueError, match="wants a"):
        comp.compose(grid.plan_grid(2, 6, 7), x)
