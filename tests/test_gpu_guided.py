"""The fused colour guided filter on the GPU (csrc/guided.hip through the C ABI and through wu.guided) against tests/_guided_ref.py.

At every case of tests/_guided_cases.py the coefficient maps EQUAL the restatement's (np.array_equal: the same float64 operations in the same
order, no FMA), the uint8 outputs equal its bytes and the float outputs equal float32(q).  Outputs start as NaN (bytes: 0xA5), workspaces as
0xFF bytes (NaN doubles); whatever lies outside an image's (h, w) must still hold its fill afterwards."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest
import torch

import _guided_cases as CASES
import _guided_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FILL = 0xA5
N_COEFF, N_APPLY = 13, 11                                   # lengths of the two case lists (asserted below)


@functools.lru_cache(maxsize=None)
def _tiles():
    from wu import _lib
    lib = _lib.load()
    return lib.wu_guided_tile_h(), lib.wu_guided_tile_w()


def _same(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        raise AssertionError(f"{what}: not bit-identical: {np.mean(got != want):.1%} of the entries differ, max |diff| {np.nanmax(d)}"
                             f"{', NaN in the output' if np.isnan(d).any() else ''}")


# ---- inputs in the layouts of the case list -----------------------------------------------------------------------------------------------
def _guide_tensor(g, fmt):
    t = torch.from_numpy(g).to(DEV)
    if fmt == "contig":
        return t
    n, _, hl, wl = g.shape                                    # a crop of a larger NaN-filled NHWC buffer, seen as NCHW
    buf = torch.full((n, hl + 2, wl + 3, 3), NAN, device=DEV)
    buf[:, 1:1 + hl, 2:2 + wl] = t.permute(0, 2, 3, 1)
    v = buf[:, 1:1 + hl, 2:2 + wl].permute(0, 3, 1, 2)
    assert v.stride(1) == 1 and (not v.is_contiguous() or hl * wl == 1)
    return v


def _target_tensor(p, fmt):
    """(device tensor, the float32 values it holds)."""
    t = torch.from_numpy(p).to(DEV)
    if fmt == "nchw":
        return t, p
    if fmt == "nhwc":                                         # the sweep's (R, B, 3, H, W) output, channels-last
        v = t.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        assert v.stride(2) == 1
        return v, p
    if fmt == "bf16":
        b = t.to(torch.bfloat16)
        return b, b.float().cpu().numpy()                     # float32 holds the bfloat16 values exactly
    r, n, _, hl, wl = p.shape                                 # a strided slice of a larger NaN-filled tensor
    buf = torch.full((r + 1, n, 3, hl + 3, wl + 5), NAN, device=DEV)
    buf[1:, :, :, 2:2 + hl, 1:1 + wl] = t
    return buf[1:, :, :, 2:2 + hl, 1:1 + wl], p


@functools.lru_cache(maxsize=None)
def _coeff_case(i):
    case = CASES.coefficient_cases(*_tiles())[i]
    g, p = CASES.case_inputs(case, 100 + i)
    pt, pvals = _target_tensor(p, case["tfmt"])
    want = R.coefficients(g, pvals, case["r"], case["eps"])
    want.setflags(write=False)
    return case, _guide_tensor(g, case["gfmt"]), pt, want


@functools.lru_cache(maxsize=None)
def _apply_case(i):
    case = CASES.apply_cases(*_tiles())[i]
    g, p = CASES.case_inputs(case, 200 + i)
    co = R.coefficients(g, p, 1, 1e-3)
    photos = CASES.photo_batch(case["sizes"], 300 + i)
    u8, f32 = R.apply_batch(co, photos, case["sizes"], FILL)
    for a in (co, photos, u8, f32):
        a.setflags(write=False)
    return case, co, photos, u8, f32


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def _abi_coeffs(g, p, r, eps, g_range=(-1, 1), t_range=(0, 1)):
    from wu import _lib
    lib = _lib.load()
    rows, n, _, hl, wl = p.shape
    nbytes = lib.wu_guided_workspace_bytes(n, rows, hl, wl)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((rows, n, 12, hl, wl), NAN, dtype=torch.float64, device=DEV)
    code = {torch.float32: 0, torch.bfloat16: 1}[p.dtype]
    _lib.call("wu_guided_coeffs", g.data_ptr(), *g.stride(), *R.range_mapping(g_range), p.data_ptr(), *p.stride(), code,
              *R.range_mapping(t_range), n, rows, hl, wl, r, eps, ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _abi_apply(co, photos, sizes, kind):
    from wu import _lib
    rows, n, _, hl, wl = co.shape
    hmax, wmax = photos.shape[1:3]
    cd, pd = torch.from_numpy(np.array(co)).to(DEV), torch.from_numpy(np.array(photos)).to(DEV)
    flat = [int(v) for s in sizes for v in s]
    host = (ctypes.c_int * len(flat))(*flat)
    sd = torch.tensor(flat, dtype=torch.int32, device=DEV)
    if kind == "uint8":
        out = torch.full((rows, n, hmax, wmax, 3), FILL, dtype=torch.uint8, device=DEV)
        ptrs = (out.data_ptr(), None)
    else:
        out = torch.full((rows, n, 3, hmax, wmax), NAN, dtype=torch.float32, device=DEV)
        ptrs = (None, out.data_ptr())
    _lib.call("wu_guided_apply", cd.data_ptr(), n, rows, hl, wl, pd.data_ptr(), hmax, wmax, host, sd.data_ptr(), *ptrs,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_f32(got, want, what):
    """Float outputs: NaN exactly where the reference has its fill (outside the images), equal bits elsewhere."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: padding written or pixels left unwritten"
    _same(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0), what)


def test_case_lists_have_the_lengths_the_parametrisation_uses():
    assert len(CASES.coefficient_cases(*_tiles())) == N_COEFF and len(CASES.apply_cases(*_tiles())) == N_APPLY


@pytest.mark.parametrize("i", range(N_COEFF))
def test_coefficients(i):
    from wu.guided import GuidedUpsampler
    case, g, p, want = _coeff_case(i)
    what = f"hl {case['hl']} wl {case['wl']} r {case['r']} eps {case['eps']:g} N {case['n']} R {case['rows']} {case['tfmt']} / {case['gfmt']}"
    _same(_abi_coeffs(g, p, case["r"], case["eps"]), want, f"C ABI, {what}")
    got = GuidedUpsampler(case["r"], case["eps"]).coefficients(g, p)
    assert got.dtype == torch.float64 and got.is_cuda
    _same(got.cpu().numpy(), want, f"wu.guided, {what}")


def test_targets_without_rows_and_other_ranges():
    from wu.guided import GuidedUpsampler
    case, g, p, want = _coeff_case(6)                         # 32 x 40, one image, one row, fp32 NCHW
    up = GuidedUpsampler(case["r"], case["eps"])
    got = up.coefficients(g, p[0])
    assert got.shape == want.shape[1:]
    _same(got.cpu().numpy(), want[0], "targets (N, 3, hl, wl)")
    # the network's raw output as the target: (-1, 1) -> 0.5 x + 0.5, and a guide already in (0, 1)
    g01, praw = (g * 0.5 + 0.5).contiguous(), (p * 2 - 1).contiguous()
    want2 = R.coefficients(g01.cpu().numpy(), praw.cpu().numpy(), case["r"], case["eps"], (1.0, 0.0), (0.5, 0.5))
    _same(up.coefficients(g01, praw, guide_range=(0, 1), target_range=(-1, 1)).cpu().numpy(), want2, "ranges (0, 1) / (-1, 1)")
    _same(_abi_coeffs(g01, praw, case["r"], case["eps"], (0, 1), (-1, 1)), want2, "ranges through the C ABI")


@pytest.mark.parametrize("i", range(N_APPLY))
def test_apply(i):
    from wu.guided import GuidedUpsampler
    case, co, photos, want_u8, want_f32 = _apply_case(i)
    sizes = case["sizes"]
    what = f"hl {case['hl']} wl {case['wl']} photographs {sizes} R {case['rows']}"
    _same(_abi_apply(co, photos, sizes, "uint8"), want_u8, f"C ABI uint8 (padding 0x{FILL:02X} included), {what}")
    _same_f32(_abi_apply(co, photos, sizes, "float"), want_f32, f"C ABI float, {what}")
    up = GuidedUpsampler()
    cd, pd = torch.from_numpy(np.array(co)).to(DEV), torch.from_numpy(np.array(photos)).to(DEV)
    u8, f32 = up.apply(cd, pd, sizes).cpu().numpy(), up.apply(cd, pd, sizes, out="float").cpu().numpy()
    assert u8.shape == want_u8.shape and f32.shape == want_f32.shape
    for n, (h, w) in enumerate(sizes):
        _same(u8[:, n, :h, :w], want_u8[:, n, :h, :w], f"wu.guided uint8 image {n}, {what}")
        _same(f32[:, n, :, :h, :w], want_f32[:, n, :, :h, :w], f"wu.guided float image {n}, {what}")
    if case["rows"] == 1:                                     # coefficients without rows: output without rows
        one = up.apply(cd[0], pd, sizes)
        assert one.shape == want_u8.shape[1:] and all(np.array_equal(one[n, :h, :w].cpu().numpy(), want_u8[0, n, :h, :w])
                                                      for n, (h, w) in enumerate(sizes))


def test_upsample_is_apply_of_coefficients():
    from wu.guided import GuidedUpsampler
    case = dict(hl=32, wl=40, rows=3, n=2)
    g, p = CASES.case_inputs(case, 7)
    sizes = [(97, 131), (50, 31)]
    photos = CASES.photo_batch(sizes, 7)
    up = GuidedUpsampler(r=3, eps=1e-2)
    want_u8, _ = R.apply_batch(R.coefficients(g, p, 3, 1e-2), photos, sizes)
    got = up.upsample(torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV), torch.from_numpy(photos).to(DEV), sizes).cpu().numpy()
    for n, (h, w) in enumerate(sizes):
        _same(got[:, n, :h, :w], want_u8[:, n, :h, :w], f"upsample image {n}")
    with pytest.raises(ValueError):
        up.apply(torch.zeros(1, 2, 12, 4, 4, dtype=torch.float64, device=DEV), torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV), [(9, 8), (8, 8)])
    with pytest.raises(ValueError):
        up.coefficients(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 3, 4, 5, device=DEV))


def test_runs_repeat_and_rows_equal_separate_calls():
    case, g, p, _ = _coeff_case(5)                            # 32 x 40, N 2, R 3, strided layouts
    a, b = _abi_coeffs(g, p, case["r"], case["eps"]), _abi_coeffs(g, p, case["r"], case["eps"])
    assert a.tobytes() == b.tobytes(), "two runs of wu_guided_coeffs differ"
    for r in range(case["rows"]):
        one = _abi_coeffs(g, p[r:r + 1], case["r"], case["eps"])
        assert one[0].tobytes() == a[r].tobytes(), f"row {r} of the (R, N) call differs from its own call"
    acase, co, photos, _, _ = _apply_case(7)                  # three sizes around the tile, R 3
    for kind in ("uint8", "float"):
        x, y = _abi_apply(co, photos, acase["sizes"], kind), _abi_apply(co, photos, acase["sizes"], kind)
        assert x.tobytes() == y.tobytes(), f"two runs of wu_guided_apply ({kind}) differ"
        for r in range(acase["rows"]):
            one = _abi_apply(co[r:r + 1], photos, acase["sizes"], kind)
            assert one[0].tobytes() == x[r].tobytes(), f"{kind}: row {r} of the (R, N) call differs from its own call"


def test_graph_capture_replays_to_the_same_bits():
    from wu.guided import GuidedUpsampler
    case = dict(hl=32, wl=40, rows=3, n=2)
    g, p = CASES.case_inputs(case, 9)
    sizes = [(65, 70), (33, 129)]
    gd, pd, ph = torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV), torch.from_numpy(CASES.photo_batch(sizes, 9)).to(DEV)
    up = GuidedUpsampler()
    want = up.coefficients(gd, pd).clone()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        up.coefficients(gd, pd)                               # warm-up on the capture stream: the workspace exists
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        got = up.coefficients(gd, pd)
    got.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    want_u8, _ = R.apply_batch(want.cpu().numpy(), ph.cpu().numpy(), sizes)
    u8 = up.apply(got, ph, sizes).cpu().numpy()
    for n, (h, w) in enumerate(sizes):
        _same(u8[:, n, :h, :w], want_u8[:, n, :h, :w], f"image {n}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _net(nc):
    import cunet
    torch.manual_seed(3)
    return cunet.Conditional_UNet(nc, precision="fp32").to(DEV).eval()


def test_transfer_fullres_equals_the_steps_by_hand(golden_dir):
    from wu import infer_driver as D
    from wu.guided import GuidedUpsampler
    from wu.input_pipeline import GPUInputPipeline
    from wu.jpeg import GPUJpegDecoder
    files = [os.path.join(golden_dir, "jpeg", f) for f in ("baseline_420.jpg", "s440.jpg")]          # 52 x 70 and 32 x 32 (h == hl)
    nc, S = 4, 32
    net = _net(nc)
    rows = torch.tensor([[1.0, 0, 0, 0], [0.1, 0.2, -0.5, 0.9]], device=DEV)
    dec = GPUJpegDecoder()
    try:
        photos, sizes = dec.decode_batch(files)
    finally:
        dec.close()
    assert sorted(sizes) == [(32, 32), (52, 70)]
    got = D.transfer_fullres(net, photos, sizes, rows, S, upsampler=GuidedUpsampler(r=2, eps=1e-3))
    assert got.shape == (2, 2, 52, 70, 3) and got.dtype == torch.uint8 and got.is_cuda
    with torch.no_grad():
        batch = GPUInputPipeline(S, train=False)(photos, sizes)
        out = net.sweep(batch, rows, batch.shape[0])
        low = D.normalize_minmax(out.reshape(-1, 3, S, S)).view(out.shape)
    co = R.coefficients(batch.cpu().numpy(), low.cpu().numpy(), 2, 1e-3)
    want, _ = R.apply_batch(co, photos.cpu().numpy(), sizes)
    for n, (h, w) in enumerate(sizes):
        _same(got[:, n, :h, :w].cpu().numpy(), want[:, n, :h, :w], f"transfer_fullres image {n} ({h} x {w})")
    # normalize=False: (out + 1) / 2 as the target; one row per image as (1, N, nc)
    got2 = D.transfer_fullres(net, photos, sizes, rows[None, :, :], S, normalize=False, upsampler=GuidedUpsampler(r=2, eps=1e-3))
    with torch.no_grad():
        out2 = net.sweep(batch, rows[None, :, :], batch.shape[0])
    want2, _ = R.apply_batch(R.coefficients(batch.cpu().numpy(), ((out2 + 1) / 2).cpu().numpy(), 2, 1e-3), photos.cpu().numpy(), sizes)
    for n, (h, w) in enumerate(sizes):
        _same(got2[:, n, :h, :w].cpu().numpy(), want2[:, n, :h, :w], f"normalize=False, rows per image, image {n}")


def test_fullres_sweep_to_dir_writes_files_of_the_photographs_sizes(golden_dir, tmp_path):
    from PIL import Image
    from wu import infer_driver as D
    from wu.jpeg import GPUJpegDecoder
    from wu.png_enc import GPUPngEncoder
    files = [os.path.join(golden_dir, "jpeg", f) for f in ("baseline_420.jpg", "s440.jpg")]
    names = ["sun", "rain", "snow"]
    net = _net(len(names))
    dec = GPUJpegDecoder()
    try:
        photos, sizes = dec.decode_batch(files)
        written = D.fullres_sweep_to_dir(net, files, [2, 0], names, tmp_path / "jpg", input_size=32, decoder=dec)
    finally:
        dec.close()
    assert [os.path.basename(p) for p in written] == [f"{src}_{stem}_{dst}.jpg" for dst in names
                                                      for src, stem in (("snow", "baseline_420"), ("sun", "s440"))]
    want = D.transfer_fullres(net, photos, sizes, torch.eye(3, device=DEV), 32).cpu().numpy()
    for k, path in enumerate(written):
        i, j = divmod(k, 2)
        h, w = sizes[j]
        with Image.open(path) as im:
            assert im.size == (w, h) and im.mode == "RGB"
        buf = io.BytesIO()
        Image.fromarray(want[i, j, :h, :w]).save(buf, "JPEG")                # what save_images guarantees: Pillow's encoding of the same bytes
        assert open(path, "rb").read() == buf.getvalue(), f"{os.path.basename(path)} differs from Pillow's encoding of the same bytes"
    # lossless: the GPU PNG encoder and Pillow's own PNG writer hold exactly the bytes of transfer_fullres
    enc = GPUPngEncoder()
    try:
        gpu_png = D.fullres_sweep_to_dir(net, files, None, names, tmp_path / "png", input_size=32, ext=".png", png_encoder=enc)
    finally:
        enc.close()
    pil_png = D.fullres_sweep_to_dir(net, files, None, names, tmp_path / "pil", input_size=32, ext=".png")
    assert os.path.basename(gpu_png[0]) == "baseline_420_sun.png"
    for k, (a, b) in enumerate(zip(gpu_png, pil_png)):
        i, j = divmod(k, 2)
        h, w = sizes[j]
        for path in (a, b):
            assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), want[i, j, :h, :w]), path


def test_command_line_writes_what_the_driver_writes(golden_dir, tmp_path, capsys):
    import cunet
    from wu import fullres
    from wu import infer_driver as D
    from wu.guided import GuidedUpsampler
    files = [os.path.join(golden_dir, "jpeg", f) for f in ("baseline_420.jpg", "s440.jpg")]
    torch.manual_seed(5)
    net = cunet.Conditional_UNet(3, precision="bf16").to(DEV).eval()
    ckpt = tmp_path / "g.pt"
    torch.save({"inference": {k: v.detach().cpu() for k, v in net.state_dict().items()}, "discriminator": {}, "epoch": 1, "global_step": 2}, ckpt)
    assert fullres.main(["--checkpoint", str(ckpt), "--out", str(tmp_path / "cli"), "--classes", "sun,rain,snow", "--src-labels", "1,0",
                         "--size", "32", "--r", "2", "--eps", "0.01"] + files) == 0
    assert "wrote 6 files" in capsys.readouterr().out
    want = D.fullres_sweep_to_dir(net, files, [1, 0], ["sun", "rain", "snow"], tmp_path / "direct", input_size=32,
                                  upsampler=GuidedUpsampler(2, 0.01))
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(os.path.basename(p) for p in want)
    for path in want:
        assert open(path, "rb").read() == open(tmp_path / "cli" / os.path.basename(path), "rb").read(), os.path.basename(path)
    # signal rows from a .npy file, lossless output
    rows = np.array([[0.3, -0.2, 1.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    np.save(tmp_path / "rows.npy", rows)
    assert fullres.main(["--checkpoint", str(ckpt), "--out", str(tmp_path / "sig"), "--signals", str(tmp_path / "rows.npy"), "--size", "32",
                         "--png"] + files) == 0
    assert sorted(os.listdir(tmp_path / "sig")) == ["baseline_420_row0000.png", "baseline_420_row0001.png", "s440_row0000.png", "s440_row0001.png"]
    with pytest.raises(SystemExit):
        fullres.main(["--checkpoint", str(ckpt), "--out", str(tmp_path / "x")] + files)          # neither --classes nor --signals
