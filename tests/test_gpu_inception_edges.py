"""The InceptionV3 / FID kernels (csrc/inception.hip) and their host glue (wu/inception.py, wu/fid.py) where tests/test_gpu_inception.py does
not reach: H != W everywhere, the implicit-GEMM conv against an exact small-integer oracle (tests/_inception_edge_cases.py), the > 1 GiB
batch split, rectangular input resize and resize_input=False on rectangular images, pools and the global average pool on channel slices
and on maps smaller than their window, ragged feature batches.  References are float64 / int64 torch and numpy on the CPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _inception_edge_cases as C
import _inception_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _cos(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return (torch.dot(a, b) / (a.norm() * b.norm())).item()


def _assert_bf16_neighbour(got, want, what):
    """Every bf16 `got` is the largest bf16 <= want or the smallest bf16 >= want (float64 `want`): no bf16 value lies strictly between."""
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, what
    got = got.cpu()
    up = torch.nextafter(got, torch.full_like(got, INF)).double()
    down = torch.nextafter(got, torch.full_like(got, -INF)).double()
    g = got.double()
    ok = ((g <= want) & (up > want)) | ((g >= want) & (down < want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.numel()} values are not a bf16 neighbour of the float64 value; first (got, want) = " \
                     f"({g[~ok][0].item()}, {want[~ok][0].item()})"


def _slice_in(x, off, ld, dtype, fill=C.FILL):
    """(N, C, H, W) CPU tensor -> the channel slice [off, off + C) of an NHWC device buffer of ld channels, the rest holding `fill`."""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), fill, dtype=dtype, device=DEV)
    buf[..., off:off + c] = x.permute(0, 2, 3, 1).to(device=DEV, dtype=dtype)
    return buf.permute(0, 3, 1, 2)[:, off:off + c]


def _slice_out(n, c, h, w, off, ld, dtype):
    """(whole sentinel-filled NHWC buffer as (N, ld, H, W), its channel slice [off, off + c))."""
    buf = torch.full((n, h, w, ld), C.SENTINEL, dtype=dtype, device=DEV).permute(0, 3, 1, 2)
    return buf, buf[:, off:off + c]


def _assert_only_slice_written(buf, off, c, what):
    o = buf.float().cpu()
    assert torch.all(o[:, :off] == C.SENTINEL) and torch.all(o[:, off + c:] == C.SENTINEL), f"{what}: wrote outside channels [{off}, {off + c})"


# =================================================================================================
# 1. conv_kxk_kernel against the exact integer oracle
# =================================================================================================
def _pack(c, w, b, code):
    from wu import _lib
    from wu.layout import stream_ptr
    nbytes = _lib.load().wu_conv_kxk_packed_bytes(c.cout, c.cin, c.k[0], c.k[1], code)
    wp = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    wd = w.float().contiguous().to(DEV)
    _lib.call("wu_pack_conv_kxk", wd.data_ptr(), wp.data_ptr(), c.cout, c.cin_w, c.cin, c.k[0], c.k[1], code, stream_ptr())
    torch.cuda.synchronize()                      # wd may be freed once the pack has read it
    return {"w": wp, "b": b.float().contiguous().to(DEV), "k": c.k, "s": (c.s, c.s), "p": c.p, "cout": c.cout, "code": code}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", C.CONV_NAMES)
def test_conv_exact_integer_oracle(name, prec):
    """torch.equal against F.conv2d in float64 (+ bias, ReLU, one rounding to the stored dtype) on integer operands; input and output are
    channel slices of wider buffers wherever the case says so, and nothing outside the output slice is written."""
    from wu.inception import conv_kxk
    from wu.layout import precision_code
    c, dt = C.CONV_CASES[name], C.DTYPE[prec]
    x, w, b = C.operands(c)
    ho, wo = C.out_hw(c)
    xd = _slice_in(x, c.x_off, c.ldx, dt)
    buf, y = _slice_out(c.n, c.cout, ho, wo, c.y_off, c.ldy, dt)
    conv_kxk(xd, _pack(c, w, b, precision_code(prec)), y, act=c.act)
    print(name, C.branch(c, prec))
    _assert_only_slice_written(buf, c.y_off, c.cout, name)
    got, want = y.cpu(), C.expected(name, prec)
    assert torch.equal(got, want), f"{name} [{prec}]: {C.first_difference(got, want)}"


# =================================================================================================
# 2. the > 1 GiB batch split and the guard beside it
# =================================================================================================
def test_conv_batch_split_over_one_gib():
    """65 images of 16 MiB (a 16-channel slice of a 2048-channel fp32 buffer): wu_conv_kxk_fwd issues one launch of 64 images and one of 1,
    each with its own x, y, M and descriptor range.  Exact integer oracle; then the 'too large' guard for a single 1 GiB image."""
    from wu import _lib
    from wu.inception import conv_kxk
    from wu.layout import stream_ptr
    c = C.SPLIT
    x, w, b = C.operands(c)
    want = C.expected(c.name, "fp32")
    ho, wo = C.out_hw(c)
    wide = torch.zeros((c.n, c.h, c.w, c.ldx), dtype=torch.float32, device=DEV)
    assert wide.numel() * 4 > 1 << 30
    wide[..., c.x_off:c.x_off + c.cin] = x.permute(0, 2, 3, 1).to(torch.int8).to(DEV)
    xd = wide.permute(0, 3, 1, 2)[:, c.x_off:c.x_off + c.cin]
    buf, y = _slice_out(c.n, c.cout, ho, wo, c.y_off, c.ldy, torch.float32)
    conv_kxk(xd, _pack(c, w, b, _lib.F32), y, act=c.act)
    got = y.cpu()
    del wide, xd
    torch.cuda.empty_cache()
    for n in (64, 0, 63):                          # the second launch, then the two ends of the first
        assert torch.equal(got[n], want[n]), f"image {n}: {C.first_difference(got[n:n + 1], want[n:n + 1])}"
    assert torch.equal(got, want), C.first_difference(got, want)

    # one image of H * W * ldx * 4 = 2^30 bytes: refused before any launch, so placeholders stand in for the tensors
    ph = torch.zeros(64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="too large"):
        _lib.call("wu_conv_kxk_fwd", ph.data_ptr(), 1024, ph.data_ptr(), ph.data_ptr(), ph.data_ptr(), 32, 1, 512, 512, 16, 32, 3, 3, 1, 1, 1, 1,
                  _lib.ACT_RELU, _lib.F32, stream_ptr())
    del buf, y
    torch.cuda.empty_cache()


# =================================================================================================
# 3. rectangular input resize, and the whole network without resize on rectangular images
# =================================================================================================
@pytest.mark.parametrize("n,hin,win", [(3, 375, 500), (1, 500, 375), (1, 120, 200), (3, 200, 120), (3, 64, 600), (1, 1, 7), (3, 7, 1)])
def test_prepare_rectangular(n, hin, win):
    """InceptionV3.prepare on H != W sources (down, up, mixed, degenerate) against the float64 F.interpolate: fp32 model to 1e-6 (2e-6
    through the (-1, 1) affine), bf16 model to a bf16 neighbour of the float64 value; pad channels exactly zero."""
    from wu.inception import InceptionV3
    g = torch.Generator().manual_seed(1000 * hin + win)
    u8 = torch.randint(0, 256, (n, hin, win, 3), generator=g, dtype=torch.uint8)
    f01 = torch.rand(n, 3, hin, win, generator=g)
    sources = {"u8": (u8, torch.from_numpy(u8.numpy().astype(np.float32) / 255).permute(0, 3, 1, 2)), "fp32": (f01, f01)}
    for prec in ("fp32", "bf16"):
        m = InceptionV3(precision=prec)
        for src, (inp, x01) in sources.items():
            want = R.prepare(x01)
            got = m.prepare(inp.to(DEV))
            assert got.shape == (n, 16, 299, 299) and got.dtype == C.DTYPE[prec]
            assert torch.all(got[:, 3:] == 0), (prec, src)
            if prec == "fp32":
                assert (got[:, :3].double().cpu() - want).abs().max().item() <= 1e-6, (prec, src)
            else:
                _assert_bf16_neighbour(got[:, :3], want, f"prepare {src} {hin} x {win}")
            if src == "fp32":
                got = m.prepare((x01 * 2 - 1).to(DEV), value_range=(-1, 1))
                assert torch.all(got[:, 3:] == 0)
                if prec == "fp32":
                    assert (got[:, :3].double().cpu() - want).abs().max().item() <= 2e-6
                else:
                    _assert_bf16_neighbour(got[:, :3], want, f"prepare affine {hin} x {win}")


def _smooth(n, seed, h, w):
    """Smooth random fields in [0, 1]: 4 x 4 random colour grids, bilinear to h x w."""
    g = torch.Generator().manual_seed(seed)
    return F.interpolate(torch.rand(n, 3, 4, 4, generator=g), size=(h, w), mode="bilinear", align_corners=False).clamp(0, 1)


NORESIZE_SHAPES = {(107, 139): [(64, 25, 33), (192, 11, 15), (768, 5, 7)], (139, 107): [(64, 33, 25), (192, 15, 11), (768, 7, 5)]}


@functools.lru_cache(maxsize=None)
def _noresize_reference(fid, h, w):
    """Three images and the float64 network on them, computed once per (variant, orientation); batches of 1 and 2 are its leading rows."""
    sd = R.make_params(fid, seed=11)
    x01 = _smooth(3, 12 + h, h, w)
    return sd, x01, R.forward(sd, R.prepare(x01, resize=False), fid)


def _check_noresize(fid, h, w, prec, n):
    from wu.inception import InceptionV3
    sd, x01, ref = _noresize_reference(fid, h, w)
    m = InceptionV3(output_blocks=[0, 1, 2, 3], resize_input=False, use_fid_inception=fid, precision=prec)
    m.load_state_dict(sd)
    m._check_size(h, w)
    xd = x01[:n].to(DEV)
    outs, logits = m(xd), m.logits(xd)
    shapes = [(n,) + s for s in NORESIZE_SHAPES[h, w]] + [(n, 2048, 1, 1)]
    assert [tuple(o.shape) for o in outs] == shapes
    assert [tuple(ref[i].shape[1:]) for i in range(3)] == NORESIZE_SHAPES[h, w]          # what F.conv2d / F.max_pool2d give
    assert tuple(logits.shape) == (n, R.num_classes(fid))
    errs = [_rel(outs[i].float().reshape(n, -1), ref[i][:n].reshape(n, -1)) for i in range(4)] + [_rel(logits, ref["logits"][:n])]
    coss = [_cos(outs[i].float(), ref[i][:n]) for i in range(4)] + [_cos(logits, ref["logits"][:n])]
    print(f"fid={fid} {h} x {w} {prec} N={n}: relative L2 per block + logits {['%.2e' % e for e in errs]}, cosine {['%.6f' % v for v in coss]}")
    if prec == "fp32":
        assert max(errs) <= 1e-4, errs
    else:
        assert min(coss) >= 0.999, coss


@pytest.mark.parametrize("fid", [True, False])
@pytest.mark.parametrize("h,w", [(107, 139), (139, 107)])
def test_whole_network_without_resize_rectangular(h, w, fid):
    """resize_input=False on 107 x 139 / 139 x 107: every conv and pool sees H != W, Mixed_7* runs on 2 x 3 / 3 x 2 maps.  The bars of
    test_whole_network_blocks_and_logits: fp32 relative L2 <= 1e-4 per block and for the logits, bf16 cosine >= 0.999."""
    for prec in ("fp32", "bf16"):
        _check_noresize(fid, h, w, prec, 2)
    if (h, w) == (107, 139) and fid:
        _check_noresize(True, h, w, "bf16", 1)
    if (h, w) == (139, 107) and not fid:
        _check_noresize(False, h, w, "fp32", 3)


# =================================================================================================
# 4. pools and the global average pool at their edges
# =================================================================================================
POOL_MAPS = [(1, 1, (1, 1)), (1, 1, (1, 2)), (1, 1, (2, 3)), (1, 1, (3, 2)), (1, 1, (5, 4)), (2, 0, (3, 3)), (2, 0, (4, 7)), (2, 0, (7, 4))]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ch", [4, 68])
def test_pool3x3_small_maps_on_channel_slices(ch, prec):
    """Maps down to 1 x 1 (smaller than the window), input and output as channel slices.  Max pools bit-identical to F.max_pool2d;
    averages per element: fp32 within 1e-6 * max|want|, bf16 a bf16 neighbour of the float64 average of the bf16 inputs."""
    from wu.inception import POOL_AVG, POOL_AVG_EXCL_PAD, POOL_MAX, pool3x3
    from wu.layout import precision_code
    code, dt = precision_code(prec), C.DTYPE[prec]
    g = torch.Generator().manual_seed(40 + ch)
    n, off = 3, 8
    for stride, pad, (h, w) in POOL_MAPS:
        x = torch.randn(n, ch, h, w, generator=g).to(dt)
        xd = _slice_in(x, off, ch + 12, dt, fill=1e4)
        ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
        for mode in ((POOL_MAX, POOL_AVG, POOL_AVG_EXCL_PAD) if stride == 1 else (POOL_MAX,)):
            buf, y = _slice_out(n, ch, ho, wo, off, ch + 20, dt)
            pool3x3(xd, y, stride, pad, mode, code)
            what = f"pool {h} x {w} stride {stride} pad {pad} mode {mode} C {ch} {prec}"
            _assert_only_slice_written(buf, off, ch, what)
            if mode == POOL_MAX:
                assert torch.equal(y.float().cpu(), F.max_pool2d(x.float(), 3, stride, pad)), what
                continue
            want = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=(mode == POOL_AVG))
            if prec == "fp32":
                assert (y.double().cpu() - want).abs().max().item() <= 1e-6 * want.abs().max().item(), what
            else:
                _assert_bf16_neighbour(y.contiguous(), want, what)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_global_avgpool_ragged_on_channel_slices(prec):
    """HW = 1, 6 (fewer pixels than the 16 pixel lanes), 15, 16, 17; C = 4, 68, 192; the input a slice with ldx > C."""
    from wu.inception import global_avgpool
    from wu.layout import precision_code
    code, dt = precision_code(prec), C.DTYPE[prec]
    g = torch.Generator().manual_seed(50)
    for ch in (4, 68, 192):
        for h, w in ((1, 1), (2, 3), (3, 5), (2, 8), (17, 1)):
            x = torch.randn(3, ch, h, w, generator=g).to(dt)
            feat = global_avgpool(_slice_in(x, 8, ch + 24, dt, fill=1e4), code)
            want = x.double().mean(dim=(2, 3))
            assert feat.dtype == torch.float32 and tuple(feat.shape) == (3, ch)
            assert (feat.double().cpu() - want).abs().max().item() <= 1e-6 * want.abs().max().item(), (ch, h, w)


def test_fid_statistics_update_averages_a_bf16_block():
    """FIDStatistics.update through a block-1 (192-channel) bf16 model, no resize, 35 x 43 images (2 x 3 maps): the FID of two image sets
    against the FID from update_features of the float64 reference's spatial means -- the bar of test_fid_end_to_end_and_cli."""
    from wu.fid import FIDStatistics, calculate_frechet_distance
    from wu.inception import InceptionV3
    sd = R.make_params(True, seed=6)
    base = _smooth(256, 7, 35, 43)
    shift = torch.tensor([0.15, -0.1, 0.05]).view(1, 3, 1, 1)
    model = InceptionV3([1], resize_input=False, precision="bf16")
    model.load_state_dict(sd)
    got, ref = [], []
    for x01 in (base, (base + shift).clamp(0, 1)):
        st, sr = FIDStatistics(model), FIDStatistics(None)
        for i in range(0, 256, 50):                                  # the last batch has 6 images
            st.update(x01[i:i + 50].to(DEV))
            feats = R.forward(sd, R.prepare(x01[i:i + 50], resize=False), True, last=1)[1].mean(dim=(2, 3))
            sr.update_features(feats.float().to(DEV))
        assert st.n == sr.n == 256
        got.append(st.finalize())
        ref.append(sr.finalize())
    fid_got = calculate_frechet_distance(*got[0], *got[1])
    fid_ref = calculate_frechet_distance(*ref[0], *ref[1])
    print(f"FID dims=192 bf16: update {fid_got:.8f}, update_features of the float64 reference {fid_ref:.8f}")
    assert fid_ref > 0 and abs(fid_got - fid_ref) <= 1e-3 * fid_ref


# =================================================================================================
# 5. ragged feature statistics
# =================================================================================================
def _gpu_stats(rows, batches, ld_extra=24, off=8):
    """FIDStatistics over `rows` fed in `batches`, every batch a column slice of a wider device tensor (stride(0) > D)."""
    from wu.fid import FIDStatistics
    st = FIDStatistics(None)
    for xb in C.split_rows(rows, batches):
        wide = torch.full((xb.shape[0], xb.shape[1] + ld_extra), 1e6, dtype=torch.float32, device=DEV)
        wide[:, off:off + xb.shape[1]] = torch.from_numpy(xb).to(DEV)
        view = wide[:, off:off + xb.shape[1]]
        assert view.stride(0) > xb.shape[1] and view.stride(1) == 1
        st.update_features(view)
    return st


@pytest.mark.parametrize("d", C.STAT_DIMS)
def test_feature_statistics_ragged_batches(d):
    """Batches of any size (odd, 1) and widths off the 64-wide tile against np.mean / np.cov in float64: the bar of
    test_feature_statistics_against_numpy.  A constant column has variance and covariances exactly 0; equal columns give equal rows."""
    from wu.fid import FIDStatistics
    for k, batches in enumerate(C.STAT_BATCHES):
        rows = C.stat_rows(sum(batches), d, 100 * d + k)
        mu, sigma = _gpu_stats(rows, batches).finalize()
        want_mu, want_s = C.float64_stats(rows)
        what = (d, batches)
        assert mu.shape == (d,) and sigma.shape == (d, d)
        assert np.abs(mu - want_mu).max() <= 1e-6 * np.abs(want_mu).max(), what
        assert np.abs(sigma - want_s).max() <= 1e-6 * np.abs(want_s).max(), (what, np.abs(sigma - want_s).max() / np.abs(want_s).max())
        assert mu[C.CONST_COL] == rows[0, C.CONST_COL]
        assert np.all(sigma[C.CONST_COL] == 0.0) and np.all(sigma[:, C.CONST_COL] == 0.0), what
        i, j = C.TWIN_COLS
        assert np.array_equal(sigma[i], sigma[j]) and np.array_equal(sigma[:, i], sigma[:, j]) and mu[i] == mu[j], what
    st = FIDStatistics(None)
    st.update_features(torch.from_numpy(C.stat_rows(1, d, 0)).to(DEV))
    with pytest.raises(ValueError, match="at least 2"):
        st.finalize()


def test_feature_statistics_need_the_shift():
    """Column means of 1e3 with deviations 0.01 .. 2 (D = 72, batches 50, 50, 1): the GPU's worst error of mu / sigma, relative to the
    largest float64 entry, stays within 4 x the error of a numpy emulation of the kernel's arithmetic (C.emulate_stats).  Measured:
    emulation 7.61e-08, hence the bound 3.05e-07; an unshifted fp32 accumulation of the same rows errs by 1.18e-01 (asserted at import of
    the case module to miss the bound)."""
    assert C.STRESS_UNSHIFTED_ERROR > C.STRESS_BOUND
    mu, sigma = _gpu_stats(C.STRESS_ROWS, C.STRESS_BATCHES).finalize()
    err = C.stats_error(mu, sigma, *C.float64_stats(C.STRESS_ROWS))
    print(f"stress statistics: GPU {err:.3e}, emulation {C.STRESS_EMULATION_ERROR:.3e}, bound {C.STRESS_BOUND:.3e}, "
          f"unshifted fp32 {C.STRESS_UNSHIFTED_ERROR:.3e}")
    assert err <= C.STRESS_BOUND
