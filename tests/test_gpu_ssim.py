"""SSIM / MS-SSIM / PSNR on the GPU (csrc/ssim.hip through the C ABI and through wu.paired) against tests/_ssim_ref.py.

At every shape: the level-0 ssim map EQUALS the restatement's (same operations in the same order, no FMA: reversing the tap order alone
changes 92 % of a 224 x 224 map); every ssim / cs mean is within 2 N 2^-53 of the restatement's, N the map's entry count (_ssim_ref.mean_bound:
derived, not measured); sse / sae equal an int64 oracle for uint8 inputs and are within N 2^-53 relative for float ones (non-negative terms
summed in any order).  Outputs start as NaN and the workspace as 0xFF bytes (NaN doubles).

combine_ssim / combine_ms_ssim run on the kernel's own means against numpy's ``**`` on those same means -- the device pow against numpy's.
Largest relative difference observed over the case list of test_combinations_against_numpy_pow on an MI355X: 3.338e-16 (MS-SSIM at
161 x 161; SSIM at most 2.5e-16, at 224 x 224); the tolerance is 8 x that, 2.67e-15."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _ssim_cases as CASES
import _ssim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
COMBINE_OBSERVED = 3.338e-16
COMBINE_TOL = 8 * COMBINE_OBSERVED


def _tiles():
    from wu import _lib
    lib = _lib.load()
    return lib.wu_ssim_tile_h(), lib.wu_ssim_tile_w()


def _abi(x, y, value_range=(-1, 1), k=11, levels=1, want_map=True):
    """wu_ssim_pairs called directly on CUDA tensors x (B, C, H, W), y (R, B, C, H, W) of any strides; numpy results."""
    from wu import _lib
    lib = _lib.load()
    code = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}[x.dtype]
    b, c, h, w = x.shape
    r = y.shape[0]
    scale, shift, L = R.range_mapping(value_range)
    nbytes = lib.wu_ssim_workspace_bytes(b, r, c, h, w, k, levels)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    sm = torch.full((r, b, c, levels), NAN, dtype=torch.float64, device=DEV)
    cm = torch.full((r, b, c, levels), NAN, dtype=torch.float64, device=DEV)
    err = torch.full((r, b, 2), NAN, dtype=torch.float64, device=DEV)
    mp = torch.full((r, b, c, h - k + 1, w - k + 1), NAN, dtype=torch.float64, device=DEV) if want_map else None
    win = (ctypes.c_double * k)(*R.gaussian_window(k).tolist())
    _lib.call("wu_ssim_pairs", x.data_ptr(), *x.stride(), y.data_ptr(), *y.stride(), code, b, r, c, h, w, scale, shift, L, 0.01, 0.03, win, k,
              levels, ws.data_ptr(), sm.data_ptr(), cm.data_ptr(), err.data_ptr(), mp.data_ptr() if want_map else None,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {"ssim_mean": sm.cpu().numpy(), "cs_mean": cm.cpu().numpy(), "err": err.cpu().numpy(), "ssim_map": mp.cpu().numpy() if want_map else None}


def _paired(x, y, value_range=(-1, 1), k=11, levels=1, want_map=True):
    from wu import paired
    st = paired.pair_stats(x, y, value_range, k, levels=levels, return_map=want_map)
    assert st.ssim_mean.dtype == torch.float64 and st.ssim_mean.is_cuda
    return {"ssim_mean": st.ssim_mean.cpu().numpy(), "cs_mean": st.cs_mean.cpu().numpy(), "err": st.err.cpu().numpy(),
            "ssim_map": st.ssim_map.cpu().numpy() if want_map else None}


def _check(got, ref, what, exact_err):
    """The module docstring's requirements on one call's outputs."""
    if got["ssim_map"] is not None:
        g, w = got["ssim_map"], ref["ssim_map"]
        assert g.shape == w.shape and np.array_equal(g, w), \
            f"{what}: level-0 ssim map not bit-identical: {np.mean(g != w):.1%} of the entries differ, max |diff| {np.nanmax(np.abs(g - w))}"
    levels = ref["ssim_mean"].shape[-1]
    h, w = ref["ssim_map"].shape[-2:]
    k = ref["k"]
    sizes = R.pooled_sizes(h + k - 1, w + k - 1, levels)
    for l in range(levels):
        n = (sizes[l][0] - k + 1) * (sizes[l][1] - k + 1)
        for name in ("ssim_mean", "cs_mean"):
            d = np.abs(got[name][..., l] - ref[name][..., l]).max()
            print(f"{what}: level {l} ({n} entries) {name} max |diff| {d:.2e}, bound {R.mean_bound(n):.2e}")
            assert d <= R.mean_bound(n), f"{what}: {name} of level {l} off by {d}"
    for i, name in enumerate(("sse", "sae")):
        g, w = got["err"][..., i], ref[name]
        if exact_err:
            assert np.array_equal(g, w.astype(np.float64)), f"{what}: {name} {g} != int64 oracle {w}"
        else:
            assert np.all(np.abs(g - w) <= ref["numel"] * R.U * np.abs(w)), f"{what}: {name} {g} vs {w}"


def _as5(y):
    return y if y.ndim == 5 else y[None]


def _ref(x, y, value_range=(-1, 1), k=11, levels=1):
    """The restatement on numpy inputs with y as (R, B, C, H, W); uint8 error sums from int64."""
    st = R.pair_stats(x, y, value_range, k, levels=levels)
    st["k"] = k
    if x.dtype == np.uint8:
        d = x.astype(np.int64) - y.astype(np.int64)
        st["sse"], st["sae"] = (d * d).sum(axis=(-3, -2, -1)), np.abs(d).sum(axis=(-3, -2, -1))
    return st


@functools.lru_cache(maxsize=None)
def _float_case(b, r, c, h, w, k, levels, seed):
    x, y = CASES.pair((b, c, h, w), seed, rows=r)
    return x, y, _ref(x, y, k=k, levels=levels)


def _cuda(a, dtype=None):
    t = torch.from_numpy(a).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("case", range(6))
def test_single_scale_shapes_c_abi(case):
    h, w, k = CASES.single_scale_shapes(*_tiles())[case]
    x, y, ref = _float_case(2, 2, 2, h, w, k, 1, seed=h * 100 + w)
    _check(_abi(_cuda(x), _cuda(y), k=k), ref, f"{h}x{w} k {k}", False)


@pytest.mark.parametrize("b,r,c", [(1, 1, 1), (1, 1, 3)])
def test_one_image_one_row(b, r, c):
    th, tw = _tiles()
    x, y, ref = _float_case(b, r, c, th + 9, tw + 13, 11, 1, seed=c)
    _check(_abi(_cuda(x), _cuda(y)), ref, f"B {b} R {r} C {c}", False)
    got = _paired(_cuda(x), _cuda(y)[0])                                     # y without the leading R: outputs without it too
    assert got["ssim_mean"].shape == (b, c, 1) and got["err"].shape == (b, 2)
    assert np.array_equal(got["ssim_map"], ref["ssim_map"][0])


@pytest.mark.parametrize("h,w,k", CASES.MS_SHAPES, ids=lambda v: str(v))
def test_multi_scale_shapes(h, w, k):
    x, y, ref = _float_case(2, 2, 2, h, w, k, 5, seed=h + w)
    assert R.pooled_sizes(h, w)[-1][0] - k + 1 == 1                          # the last map is a single row
    _check(_abi(_cuda(x), _cuda(y), k=k, levels=5), ref, f"MS {h}x{w} k {k}", False)


def test_224_three_rows_through_wu_paired():
    from wu import paired
    x, y, ref = _float_case(2, 3, 3, 224, 224, 11, 5, seed=224)
    xd, yd = _cuda(x), _cuda(y)
    _check(_paired(xd, yd, levels=5), ref, "224x224 B 2 R 3 C 3", False)
    m = paired.paired_metrics(xd, yd)
    assert all(v.shape == (3, 2) and v.dtype == torch.float64 and v.is_cuda for v in m)
    assert np.abs(m.ssim.cpu().numpy() - R.combine_ssim(ref)).max() <= R.mean_bound(214 * 214)
    # ms = prod v_l^w_l: a relative error of at most sum_l w_l mean_bound(N_l) / v_l from the means, and a few 2^-53 from pow and the product
    v = R.ms_values(ref["ssim_mean"], ref["cs_mean"])
    sizes = R.pooled_sizes(224, 224)
    rel = sum(wl * R.mean_bound((s[0] - 10) * (s[1] - 10)) / v[..., l].min() for l, (wl, s) in enumerate(zip(R.MS_WEIGHTS, sizes)))
    assert v.min() > 0.1 and np.abs(m.ms_ssim.cpu().numpy() - R.combine_ms_ssim(ref)).max() <= rel + 64 * R.U
    # sse and sae within numel 2^-53 relative: psnr moves by 10 / ln 10 times that, mae by that
    tol = ref["numel"] * R.U
    assert np.abs(m.psnr.cpu().numpy() - R.psnr(ref)).max() <= 10 / np.log(10) * tol + 64 * R.U * R.psnr(ref).max()
    assert np.all(np.abs(m.mae.cpu().numpy() - R.mae(ref)) <= (tol + 2 * R.U) * R.mae(ref))
    assert torch.equal(paired.ssim(xd, yd), m.ssim) and torch.equal(paired.ms_ssim(xd, yd), m.ms_ssim) and torch.equal(paired.psnr(xd, yd), m.psnr)
    assert paired.paired_metrics(xd, yd, ms=False).ms_ssim is None
    with pytest.raises(ValueError, match="MS-SSIM"):
        paired.ms_ssim(xd[..., :160, :], yd[..., :160, :])


def test_identical_images_on_the_device():
    from wu import paired
    x, _, _ = _float_case(2, 3, 3, 224, 224, 11, 5, seed=224)
    xd = _cuda(x)
    st = paired.pair_stats(xd, xd.clone(), levels=5, return_map=True)
    assert torch.all(st.ssim_map == 1.0) and torch.all(st.ssim_mean == 1.0) and torch.all(st.cs_mean == 1.0) and torch.all(st.err == 0.0)
    assert torch.all(torch.isposinf(paired.psnr_of(st))) and torch.all(paired.combine_ms_ssim(st) == 1.0)


def test_bf16_inputs():
    th, tw = _tiles()
    x, y = CASES.pair((2, 3, th + 11, tw + 9), seed=16, rows=2)
    xb, yb = _cuda(x, torch.bfloat16), _cuda(y, torch.bfloat16)
    ref = _ref(xb.float().cpu().numpy(), yb.float().cpu().numpy())            # float32 holds the bfloat16 values exactly
    _check(_abi(xb, yb), ref, "bf16", False)
    _check(_paired(xb, yb), ref, "bf16 wu.paired", False)
    _check(_paired(xb.float(), yb), ref, "fp32 x against bf16 y", False)      # differing float dtypes: both widened, the same numbers


@pytest.mark.parametrize("h,w,k,levels", [(43, 41, 11, 1), (33, 35, 3, 5)])
def test_uint8_nhwc_permuted_view(h, w, k, levels):
    x, y = CASES.pair_u8((2, 3, h, w), seed=8, rows=2)
    ref = _ref(x, y, "uint8", k, levels)
    xd = _cuda(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)           # NHWC storage, as the decoders return it
    yd = _cuda(np.ascontiguousarray(y.transpose(0, 1, 3, 4, 2))).permute(0, 1, 4, 2, 3)
    assert xd.stride(1) == 1 and yd.stride(2) == 1
    _check(_abi(xd, yd, "uint8", k, levels), ref, f"uint8 NHWC {h}x{w}", True)
    _check(_paired(xd, yd, "uint8", k, levels), ref, f"uint8 NHWC {h}x{w} wu.paired", True)


def test_channels_last_and_crop_of_a_nan_buffer():
    th, tw = _tiles()
    h, w = th + 12, tw + 10
    x, y, ref = _float_case(2, 2, 3, h, w, 11, 1, seed=77)
    xd, yd = _cuda(x).contiguous(memory_format=torch.channels_last), _cuda(y)
    assert xd.stride(1) == 1
    _check(_paired(xd, yd), ref, "channels-last x", False)
    bx = torch.full((2, 3, h + 7, w + 5), NAN, device=DEV)
    by = torch.full((2, 2, 3, h + 3, w + 9), NAN, device=DEV)
    bx[:, :, 4:4 + h, 2:2 + w] = _cuda(x)
    by[:, :, :, 1:1 + h, 6:6 + w] = yd
    cx, cy = bx[:, :, 4:4 + h, 2:2 + w], by[:, :, :, 1:1 + h, 6:6 + w]
    assert not cx.is_contiguous() and not cy.is_contiguous()
    _check(_paired(cx, cy), ref, "crops of NaN-filled buffers", False)          # one NaN read would poison a map entry or a sum
    _check(_abi(cx, cy), ref, "crops, C ABI", False)


def test_rows_equal_separate_calls_and_runs_repeat():
    x, y, _ = _float_case(2, 3, 3, 224, 224, 11, 5, seed=224)
    xd, yd = _cuda(x), _cuda(y)
    a, b = _abi(xd, yd, levels=5), _abi(xd, yd, levels=5)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), f"two runs differ in {key}"
    for r in range(3):
        one = _abi(xd, yd[r:r + 1], levels=5)
        for key in a:
            assert one[key][0].tobytes() == a[key][r].tobytes(), f"row {r} of the (R, B) call differs from its own call in {key}"


@pytest.mark.parametrize("b,c,r", [(16, 64, 3), (8, 64, 3), (2, 2, 5)])
def test_rows_walked_by_one_workgroup_and_split_over_several(b, c, r):
    """The library splits the R rows over workgroups while B C tiles stays under 1024 and lets one workgroup walk them otherwise: 1024 tiles
    walk all three rows (each prefetched behind the previous one), 512 tiles walk rows (0, 1) and (2), 4 tiles take one row each."""
    x, y, ref = _float_case(b, r, c, 13, 14, 3, 1, seed=b + c)
    xd, yd = _cuda(x), _cuda(y)
    got = _abi(xd, yd, k=3)
    _check(got, ref, f"B {b} C {c} R {r}", False)
    last = _abi(xd, yd[r - 1:], k=3)
    for key in got:
        assert last[key][0].tobytes() == got[key][r - 1].tobytes(), key


def test_graph_capture_replays_to_the_same_bits():
    from wu import paired
    x, y, _ = _float_case(2, 2, 2, 33, 35, 3, 5, seed=68)
    xd, yd = _cuda(x), _cuda(y)
    want = paired.pair_stats(xd, yd, win_size=3, levels=5, return_map=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        paired.pair_stats(xd, yd, win_size=3, levels=5, return_map=True)       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        got = paired.pair_stats(xd, yd, win_size=3, levels=5, return_map=True)
    for t in got[:4]:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(got[:4], want[:4]):
        assert torch.equal(g, w)


def test_combinations_against_numpy_pow():
    """combine_ssim / combine_ms_ssim on the kernel's own means against numpy on those same means: what differs is torch's device pow and
    product against numpy's.  Prints the largest relative difference; COMBINE_OBSERVED records it, the tolerance is 8 x that."""
    from wu import paired
    worst = 0.0
    cases = [(h, w, k, (-1, 1)) for h, w, k in CASES.MS_SHAPES] + [(224, 224, 11, (-1, 1)), (40, 40, 3, (0, 1))]
    for h, w, k, vr in cases:
        if vr == (0, 1):
            x = np.random.RandomState(6).rand(1, 1, 40, 40).astype(np.float32)
            x, y = x, (1.0 - x)[None]                                           # negative cs means: the clamp, MS-SSIM exactly 0
        else:
            x, y, _ = _float_case(2, 3, 3, h, w, k, 5, seed=224) if h == 224 else _float_case(2, 2, 2, h, w, k, 5, seed=h + w)
        st = paired.pair_stats(_cuda(x), _cuda(y), vr, k, levels=5)
        sm, cm = st.ssim_mean.cpu().numpy(), st.cs_mean.cpu().numpy()
        want_s = sm[..., 0].mean(-1)
        want_m = (np.maximum(R.ms_values(sm, cm), 0.0) ** np.asarray(R.MS_WEIGHTS)).prod(-1).mean(-1)
        got_s, got_m = paired.combine_ssim(st).cpu().numpy(), paired.combine_ms_ssim(st).cpu().numpy()
        if vr == (0, 1):
            assert np.all(cm[0, 0, 0, :4] < 0) and got_m[0, 0] == 0.0 and want_m[0, 0] == 0.0
            assert paired.combine_ssim(st, nonnegative=True)[0, 0].item() == 0.0 and got_s[0, 0] < 0
        for got, want in ((got_s, want_s), (got_m, want_m)):
            rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
            rel = np.where(want == got, 0.0, rel)
            worst = max(worst, float(rel.max()))
            print(f"{h}x{w} k {k}: combine max relative difference {rel.max():.3e}")
    print(f"largest relative difference over the case list: {worst:.3e} (recorded: {COMBINE_OBSERVED:.1e})")
    assert worst <= COMBINE_TOL


def test_cli_on_two_directories(tmp_path, capsys):
    from PIL import Image
    from wu import paired
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    xs, ys = CASES.pair_u8((3, 3, 36, 40), seed=2)
    xl, yl = CASES.pair_u8((2, 3, 40, 36), seed=3)
    for i, (p, q) in enumerate(list(zip(xs, ys)) + list(zip(xl, yl))):
        Image.fromarray(p.transpose(1, 2, 0)).save(a / f"im{i}.png")
        Image.fromarray(q.transpose(1, 2, 0)).save(b / f"im{i}.png")
    assert paired.main([str(a), str(b), "--win", "3", "--batch-size", "2"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["SSIM", "MS-SSIM", "PSNR", "MAE", "pairs"] and lines[-1] == "pairs: 5"
    refs = [_ref(xs, ys, "uint8", 3, 5), _ref(xl, yl, "uint8", 3, 5)]
    want_ssim = np.concatenate([R.combine_ssim(s) for s in refs]).mean()
    want_ms = np.concatenate([R.combine_ms_ssim(s) for s in refs]).mean()
    want_psnr = np.concatenate([R.psnr(s) for s in refs]).mean()
    want_mae = np.concatenate([R.mae(s) for s in refs]).mean()
    got = [float(ln.split(":")[1].split()[0]) for ln in lines[:4]]
    assert abs(got[0] - want_ssim) <= 1e-6 and abs(got[1] - want_ms) <= 1e-6 and abs(got[2] - want_psnr) <= 1e-4 and abs(got[3] - want_mae) <= 1e-6
    assert paired.main([str(a), str(b), "--no-ms"]) == 0
    assert len(capsys.readouterr().out.strip().splitlines()) == 4
    Image.fromarray(xs[0].transpose(1, 2, 0)[:30]).save(b / "im0.png")
    with pytest.raises(ValueError, match="40 x 30"):
        paired.main([str(a), str(b), "--win", "3"])


def test_transfer_evaluations_with_content():
    """content= changes nothing in what the evaluations computed before, and ContentPreservation.result() is paired_metrics of the sweep."""
    import cunet
    from wu import paired
    from wu.evaluate import ClassTransferEval, ContentPreservation, EstimatorTransferEval
    from wu.train_step import StandInEstimator
    nc, b = 5, 3
    torch.manual_seed(0)
    net = cunet.Conditional_UNet(nc, precision="bf16").to(DEV).eval()
    torch.manual_seed(11)
    est = StandInEstimator(nc).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand((b, 3, 64, 64), generator=g) * 2 - 1).to(DEV) for _ in range(2)]
    ref_rows = torch.randn((2, nc), generator=g).to(DEV)
    content = ContentPreservation(ms=True, win_size=3)                         # 64 > 16 (3 - 1): MS-SSIM is legal with the 3-tap window
    plain, with_c = ClassTransferEval(net, est, nc), ClassTransferEval(net, est, nc, content=content)
    sums = torch.zeros(nc, 4, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        for batch in batches:
            plain.update(batch)
            with_c.update(batch)
            fakes = net.sweep(batch, torch.eye(nc, device=DEV), with_c.max_images)
            m = paired.paired_metrics(batch, fakes, win_size=3)
            mse = paired.mse_of(paired.pair_stats(batch, fakes, win_size=3))
            sums += torch.stack([m.ssim.sum(1), m.ms_ssim.sum(1), mse.sum(1), m.mae.sum(1)], -1)
    assert torch.equal(plain.confusion(), with_c.confusion()) and int(plain.confusion().sum()) == 2 * nc * b
    res = content.result()
    want = (sums / (2 * b)).cpu()
    assert res["count"] == 2 * b and all(res[key].shape == (nc,) for key in ("ssim", "ms_ssim", "mse", "mae", "psnr"))
    for i, key in enumerate(("ssim", "ms_ssim", "mse", "mae")):               # the same six numbers per row, added in another order
        assert torch.all((res[key] - want[:, i]).abs() <= 8 * R.U * want[:, i].abs()), key
    assert torch.all((res["psnr"] - 10 * torch.log10(1.0 / res["mse"])).abs() <= 1e-12)
    assert torch.all(res["ssim"] < 1) and torch.all(res["ssim"] > -1) and torch.all(res["mae"] > 0)
    # the estimator sweep: the same rows of numbers with and without content, ms=False on the default window
    c2 = ContentPreservation(ms=False)
    e0, e1 = EstimatorTransferEval(net, est), EstimatorTransferEval(net, est, content=c2)
    with torch.no_grad():
        e0.update(batches[0], ref_rows)
        e1.update(batches[0], ref_rows)
        m = paired.paired_metrics(batches[0], net.sweep(batches[0], ref_rows, e1.max_images), ms=False)
    assert torch.equal(e0.all(), e1.all())
    r2 = c2.result()
    assert r2["ms_ssim"] is None and r2["count"] == b
    assert torch.all((r2["ssim"] - (m.ssim.sum(1) / b).cpu()).abs() <= 4 * R.U)
    with pytest.raises(ValueError, match="MS-SSIM"):
        ContentPreservation(ms=True).add(batches[0], net.sweep(batches[0], ref_rows, e1.max_images))
