"""LPIPS on the GPU (csrc/lpips.hip through the C ABI, wu.lpips, wu.evaluate.PerceptualDistance, the command line) against
tests/_lpips_ref.py.

Input kernel: bit-identical to the float32 restatement.  Trunk kernels at AlexNet's configurations: bit-equal to an int64 oracle.  Head and
pairs: within _lpips_ref.head_bound (derived, not measured) of the restatement; exact zeros, mirrored entries and repeated runs bit for
bit.  End to end: relative distance to the restatement with a float64 trunk within 16 x (fp32) / 4 x (bf16) the largest relative distance,
over the case list, between the restatement with a float32 (bf16-rounding) CPU trunk and with the float64 trunk; the tolerances are
computed here and printed.  Outputs start as NaN inside guarded buffers, workspaces as 0xFF bytes.

Observed on an MI355X (profiles/lpips_bench.md records them too).  Head and pairs: largest |got - ref| 1.1e-16, at most 1.1 % of the
bound.  End to end, largest relative error of the distance over the case list: fp32 3.017e-7 (pairwise 2.967e-7, diversity 1.643e-7) against
the tolerance 2.706e-6 = 16 x 1.691e-7; bf16 2.409e-3 (pairwise 1.663e-3, diversity 7.471e-4) against 9.636e-3 = 4 x 2.409e-3.  Smallest
feature-vector norm of the float64 oracle: 1.220."""
import functools

import numpy as np
import pytest
import torch

import _lpips_cases as CASES
import _lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 16
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _lib():
    from wu import _lib
    return _lib


def _tile():
    return _lib().load().wu_lpips_tile_pixels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Out:
    """n float64 outputs, NaN, inside a NaN buffer with GUARD doubles on both sides."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float64, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def numpy(self, shape):
        host = self.buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + self.n:]).all(), "wrote outside the output"
        return host[GUARD:GUARD + self.n].reshape(shape).copy()


def _nhwc(a, dtype, ld_extra=0, off=0):
    """(..., C, h, w) numpy -> device NHWC storage (a channel slice [off, off + C) of a NaN-filled buffer of C + ld_extra channels) as a
    (..., C, h, w) view."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    lead, (c, h, w) = t.shape[:-3], t.shape[-3:]
    buf = torch.full(tuple(lead) + (h, w, c + ld_extra), NAN, dtype=dtype, device=DEV)
    buf[..., off:off + c] = t.movedim(-3, -1).to(device=DEV, dtype=dtype)
    return buf[..., off:off + c].movedim(-1, -3)


def _ld(t):
    return t.stride(-1)


def _abi_head(fx, fy, w):
    """wu_lpips_head on device views fx (B, C, h, w), fy (R, B, C, h, w) (NHWC storage) -> (R, B) numpy."""
    L = _lib()
    r, b, c, h, wd = fy.shape
    nbytes = L.load().wu_lpips_workspace_bytes(b, r, h, wd, 0)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = _Out(r * b)
    code = L.F32 if fx.dtype == torch.float32 else L.BF16
    L.call("wu_lpips_head", fx.data_ptr(), _ld(fx), fy.data_ptr(), _ld(fy), fy.stride(0), w.data_ptr(), code, b, r, h, wd, c, ws.data_ptr(),
           out.view.data_ptr(), b, _stream())
    torch.cuda.synchronize()
    return out.numpy((r, b))


def _abi_pairs(f, w):
    L = _lib()
    r, b, c, h, wd = f.shape
    nbytes = L.load().wu_lpips_workspace_bytes(b, r, h, wd, 1)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = _Out(r * r * b)
    code = L.F32 if f.dtype == torch.float32 else L.BF16
    L.call("wu_lpips_pairs", f.data_ptr(), _ld(f), f.stride(0), w.data_ptr(), code, b, r, h, wd, c, ws.data_ptr(), out.view.data_ptr(), b,
           _stream())
    torch.cuda.synchronize()
    return out.numpy((r, r, b))


# =================================================================================================
# 1. the input kernel
# =================================================================================================
def _abi_input(src, value_range, prec):
    L = _lib()
    n, _, h, w = src.shape
    s, o = (float(v) for v in R.input_mapping(value_range))
    dt = DT[prec]
    per = n * h * w * 16
    buf = torch.full((per + 64,), NAN, dtype=dt, device=DEV)
    code = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}[src.dtype]
    L.call("wu_lpips_input", src.data_ptr(), *src.stride(), code, n, h, w, s, o, buf[32:].data_ptr(), L.F32 if prec == "fp32" else L.BF16,
           _stream())
    torch.cuda.synchronize()
    host = buf.float().cpu()
    assert torch.isnan(host[:32]).all() and torch.isnan(host[32 + per:]).all(), "wu_lpips_input wrote outside its output"
    return buf[32:32 + per].view(n, h, w, 16).cpu()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("h,w", CASES.INPUT_SIZES)
def test_input_kernel_bit_identical(h, w, prec):
    rng = np.random.default_rng(h * w)
    b, rows = 2, 3
    v = rng.uniform(-1, 1, size=(rows, b, 3, h, w)).astype(np.float32)
    sweep = torch.from_numpy(v).to(DEV)
    plain = sweep[0].contiguous()
    want = R.network_input(v[0], (-1, 1), prec == "bf16")
    want01 = R.network_input((v[0] + 1) / 2, (0, 1), prec == "bf16")
    big = torch.full((b, 3, h + 7, w + 5), NAN, device=DEV)
    big[:, :, 3:3 + h, 2:2 + w] = plain
    crop = big[:, :, 3:3 + h, 2:2 + w]
    cl = plain.contiguous(memory_format=torch.channels_last)
    assert cl.stride(1) == 1 and not crop.is_contiguous()
    sources = {"NCHW": plain, "channels-last": cl, "crop": crop}
    for name, src in sources.items():
        got = _abi_input(src, (-1, 1), prec)
        assert torch.all(got[..., 3:] == 0), name
        assert torch.equal(got, want), f"{name} {h}x{w} {prec}: not bit-identical"
    for r in range(rows):                                                    # the sweep's (R, B, ...) output indexed by row
        assert torch.equal(_abi_input(sweep[r], (-1, 1), prec), R.network_input(v[r], (-1, 1), prec == "bf16")), r
    assert torch.equal(_abi_input(((plain + 1) / 2), (0, 1), prec), want01)
    vb = torch.from_numpy(v[0]).to(torch.bfloat16)
    assert torch.equal(_abi_input(vb.to(DEV), (-1, 1), prec), R.network_input(vb.float().numpy(), (-1, 1), prec == "bf16"))
    u8 = rng.integers(0, 256, size=(b, h, w, 3)).astype(np.uint8)
    src = torch.from_numpy(u8).to(DEV).permute(0, 3, 1, 2)                    # NHWC storage as a permuted view
    assert src.stride(1) == 1
    got = _abi_input(src, "uint8", prec)
    assert torch.all(got[..., 3:] == 0) and torch.equal(got, R.network_input(u8.transpose(0, 3, 1, 2), "uint8", prec == "bf16"))


# =================================================================================================
# 2. the trunk kernels at AlexNet's configurations: exact
# =================================================================================================
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES.TRUNK_CONVS, ids=lambda c: c[0])
def test_trunk_conv_exact(case, prec):
    from wu.inception import conv_kxk
    from wu.layout import precision_code, stream_ptr
    L = _lib()
    name, n, h, w, cin, cin_w, cout, k, s, p = case
    x, wt, b = CASES.trunk_operands(case)
    want = CASES.trunk_expected(case)
    code, dt = precision_code(prec), DT[prec]
    wp = torch.empty(L.load().wu_conv_kxk_packed_bytes(cout, cin, k, k, code), dtype=torch.uint8, device=DEV)
    wd = wt.float().contiguous().to(DEV)
    L.call("wu_pack_conv_kxk", wd.data_ptr(), wp.data_ptr(), cout, cin_w, cin, k, k, code, stream_ptr())
    plan = {"w": wp, "b": b.float().to(DEV), "k": (k, k), "s": (s, s), "p": (p, p), "cout": cout, "code": code}
    xd = _nhwc(x.numpy().astype(np.float32), dt)
    ho, wo = want.shape[2:]
    y = torch.full((n, ho, wo, cout), NAN, dtype=dt, device=DEV).permute(0, 3, 1, 2)
    conv_kxk(xd, plan, y)
    torch.cuda.synchronize()
    stored = want.float() if prec == "fp32" else want.float().to(torch.bfloat16).float()       # the epilogue's one rounding
    got = y.float().cpu()
    assert torch.equal(got, stored), f"{name} [{prec}]: {int((got != stored).sum())} of {got.numel()} outputs differ from the int64 oracle"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_trunk_pool_exact(prec):
    from wu.inception import POOL_MAX, pool3x3
    from wu.layout import precision_code
    for n, c, h, w in CASES.TRUNK_POOLS:
        x = torch.randint(-40, 41, (n, c, h, w), generator=torch.Generator().manual_seed(c + h))
        ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        want = torch.full((n, c, ho, wo), -10 ** 9, dtype=torch.int64)
        for i in range(3):
            for j in range(3):
                want = torch.maximum(want, x[:, :, i:i + 2 * (ho - 1) + 1:2, j:j + 2 * (wo - 1) + 1:2])
        xd = _nhwc(x.numpy().astype(np.float32), DT[prec])
        y = torch.full((n, ho, wo, c), NAN, dtype=DT[prec], device=DEV).permute(0, 3, 1, 2)
        pool3x3(xd, y, 2, 0, POOL_MAX, precision_code(prec))
        torch.cuda.synchronize()
        assert torch.equal(y.float().cpu(), want.float()), (n, c, h, w, prec)


# =================================================================================================
# 3. the head through the ABI
# =================================================================================================
@functools.lru_cache(maxsize=None)
def _head_case(c, h, w, rows, bf16):
    x, y = CASES.feature_maps(c, h, w, rows, CASES.HEAD_B, seed=c * 1000 + h * 20 + w + rows)
    if bf16:
        x, y = (torch.from_numpy(a).to(torch.bfloat16).float().numpy() for a in (x, y))
    lw = CASES.lin_weight(c, c + h)
    return x, y, lw, R.head(x[None], y, lw), R.head_bound(x[None], y, lw)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("c", CASES.HEAD_CHANNELS)
def test_head_c_abi(c, prec):
    dt = DT[prec]
    for h, w in CASES.head_pixel_maps(_tile()):
        for rows in CASES.HEAD_ROWS:
            x, y, lw, ref, bound = _head_case(c, h, w, rows, prec == "bf16")
            wd = torch.from_numpy(lw).to(DEV)
            what = f"C {c} {h}x{w} R {rows} {prec}"
            # dense buffers, then channel slices of wider NaN-filled buffers (ld > C)
            for extra, off in ((0, 0), (24, 8)):
                fx, fy = _nhwc(x, dt, extra, off), _nhwc(y, dt, extra, off)
                got = _abi_head(fx, fy, wd)
                err = np.abs(got - ref)
                print(f"{what} ld C+{extra}: max |got - ref| {err.max():.3e}, bound {bound.min():.3e}")
                assert np.all(err <= bound), f"{what}: off by {err.max()} (bound {bound.max()})"
                if rows > 1:
                    assert np.all(got[0] == 0.0), f"{what}: a y row bit-equal to x must give exactly 0"
                again = _abi_head(fx, fy, wd)
                assert got.tobytes() == again.tobytes(), f"{what}: two runs differ"


def test_head_rows_do_not_depend_on_r_or_b():
    x, y, lw, _, _ = _head_case(192, 13, 13, 3, False)
    wd = torch.from_numpy(lw).to(DEV)
    fx, fy = _nhwc(x, torch.float32), _nhwc(y, torch.float32)
    got = _abi_head(fx, fy, wd)
    for r in range(3):
        assert _abi_head(fx, fy[r:r + 1], wd)[0].tobytes() == got[r].tobytes()
    assert _abi_head(fx[1:], fy[:, 1:], wd)[:, 0].tobytes() == got[:, 1].tobytes()


# =================================================================================================
# 4. pairs
# =================================================================================================
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("rows", CASES.PAIR_ROWS)
def test_pairs_c_abi(rows, prec):
    dt = DT[prec]
    t = _tile()
    for c, h, w in ((64, 3, 5), (384, 1, 1), (192, 1, t + 1)):
        x, y = CASES.feature_maps(c, h, w, rows - 1, CASES.HEAD_B, seed=rows * 7 + c)
        f = np.concatenate([x[None], y])                                        # (R, B, C, h, w): row 0 is x
        if prec == "bf16":
            f = torch.from_numpy(f).to(torch.bfloat16).float().numpy()
        lw = CASES.lin_weight(c, rows)
        wd = torch.from_numpy(lw).to(DEV)
        fd = _nhwc(f, dt, 24, 8)
        got = _abi_pairs(fd, wd)
        ref, bound = R.head(f[:, None], f[None], lw), R.head_bound(f[:, None], f[None], lw)
        what = f"pairs R {rows} C {c} {h}x{w} {prec}"
        print(f"{what}: max |got - ref| {np.abs(got - ref).max():.3e}, smallest off-diagonal bound {bound[~np.eye(rows, dtype=bool)].min():.3e}")
        assert np.all(np.abs(got - ref) <= bound), what
        assert np.all(got[np.arange(rows), np.arange(rows)] == 0.0), f"{what}: diagonal"
        assert got.tobytes() == got.transpose(1, 0, 2).copy().tobytes(), f"{what}: m[i, j] and m[j, i] differ"
        assert got.tobytes() == _abi_pairs(fd, wd).tobytes(), f"{what}: two runs differ"
        for i in range(rows - 1):                                               # both kernels form a pair the same way, whatever the row blocking
            head = _abi_head(fd[i], fd[i + 1:], wd)
            assert head.tobytes() == got[i, i + 1:].tobytes(), f"{what}: row {i} of the pair matrix is not the head's result"


# =================================================================================================
# 5. end to end through wu.lpips.LPIPS
# =================================================================================================
@functools.lru_cache(maxsize=None)
def _params():
    return R.make_params(CASES.PARAM_SEED)


@functools.lru_cache(maxsize=None)
def _e2e_reference():
    """Per case: images and the restatement with a float64, a float32 and a bf16-rounding CPU trunk; then the two tolerances."""
    alex, lin = _params()
    out, rel32, relbf, min_norm = {}, 0.0, 0.0, float("inf")
    for h, w, r in CASES.e2e_cases():
        x, fakes = CASES.images(CASES.E2E_B, r, h, w, CASES.e2e_seed(h, w, r))
        r64 = R.lpips(alex, lin, x, fakes)
        r32 = R.lpips(alex, lin, x, fakes, dtype=torch.float32)
        rbf = R.lpips(alex, lin, x, fakes, dtype=torch.float32, bf16=True)
        min_norm = min(min_norm, r64["min_norm"])
        rel32 = max(rel32, float((np.abs(r32["distance"] - r64["distance"]) / r64["distance"]).max()))
        relbf = max(relbf, float((np.abs(rbf["distance"] - r64["distance"]) / r64["distance"]).max()))
        out[h, w, r] = (x, fakes, r64)
    return out, 16 * rel32, 4 * relbf, min_norm


def _model(prec):
    from wu import lpips
    alex, lin = _params()
    m = lpips.LPIPS(prec)
    m.load_alexnet(alex)
    m.load_lin(lin)
    return m


def _rel(got, want):
    return float((np.abs(got - want) / np.abs(want)).max())


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_end_to_end(prec):
    cases, tol32, tolbf, min_norm = _e2e_reference()
    print(f"tolerances from the CPU trunks: fp32 {tol32:.3e} (16 x {tol32 / 16:.3e}), bf16 {tolbf:.3e} (4 x {tolbf / 4:.3e}); "
          f"smallest feature-vector norm of the float64 oracle {min_norm:.3f}")
    assert min_norm > 1e-3                                                    # LPIPS is discontinuous at an all-zero vector
    tol = tol32 if prec == "fp32" else tolbf
    m = _model(prec)
    worst = 0.0
    for (h, w, r), (x, fakes, ref) in cases.items():
        xd, fd = torch.from_numpy(x).to(DEV), torch.from_numpy(fakes).to(DEV)
        d, per = m.distance(xd, fd, layers=True)
        assert d.shape == (r, CASES.E2E_B) and per.shape == (r, CASES.E2E_B, 5) and d.dtype == torch.float64 and d.is_cuda
        e = _rel(d.cpu().numpy(), ref["distance"])
        el = _rel(per.cpu().numpy(), ref["layers"])
        worst = max(worst, e)
        print(f"{h}x{w} R {r} {prec}: distance relative error {e:.3e}, worst layer {el:.3e} (tolerance {tol:.3e})")
        assert e <= tol, (h, w, r, e, tol)
        one = m.distance(xd, fd[0])                                           # fakes without the leading R
        assert one.shape == (CASES.E2E_B,) and torch.equal(one, d[0])
        if r >= 2:
            pw = m.pairwise(fd)
            assert pw.shape == (r, r, CASES.E2E_B)
            off = ~np.eye(r, dtype=bool)
            ep = _rel(pw.cpu().numpy()[off], ref["pairwise"][off])
            ev = _rel(m.diversity(fd).cpu().numpy(), ref["diversity"])
            print(f"{h}x{w} R {r} {prec}: pairwise relative error {ep:.3e}, diversity {ev:.3e}")
            assert ep <= tol and ev <= tol
            assert torch.all(pw[torch.arange(r), torch.arange(r)] == 0) and torch.equal(pw, pw.transpose(0, 1))
    print(f"largest relative error of the distance over the case list [{prec}]: {worst:.3e}")


def test_identical_images_chunking_and_uint8():
    m = _model("fp32")
    x, fakes, _ = _e2e_reference()[0][67, 35, 3]
    xd, fd = torch.from_numpy(x).to(DEV), torch.from_numpy(fakes).to(DEV)
    assert torch.all(m.distance(xd, torch.stack([xd, xd.clone()])) == 0.0)    # lpips(x, x) is exactly 0
    base = m.distance(xd, fd, layers=True, max_images=64)
    pbase = m.pairwise(fd, max_images=64)
    for mi in (1, 2, 7):
        got = m.distance(xd, fd, layers=True, max_images=mi)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), f"max_images {mi} changes the bits"
        assert torch.equal(m.pairwise(fd, max_images=mi), pbase), f"pairwise: max_images {mi} changes the bits"
    # row 0 of pairwise(cat(x, fakes)) is distance(x, fakes)
    pw = m.pairwise(torch.cat([xd[None], fd]))
    assert torch.equal(pw[0, 1:], base[0])
    with pytest.raises(ValueError, match="31"):
        m.distance(xd[..., :30, :], fd[..., :30, :])
    with pytest.raises(ValueError, match="R >= 2"):
        m.pairwise(fd[:1])
    # uint8 against the float path on v * 2 / 255 - 1
    rng = np.random.default_rng(8)
    u8x = torch.from_numpy(rng.integers(0, 256, size=(2, 40, 33, 3)).astype(np.uint8)).to(DEV).permute(0, 3, 1, 2)
    u8y = torch.from_numpy(rng.integers(0, 256, size=(2, 2, 40, 33, 3)).astype(np.uint8)).to(DEV).permute(0, 1, 4, 2, 3)

    def as_float(t):
        return t.float() * float(np.float32(2.0 / 255.0)) + (-1.0)

    assert torch.equal(m.distance(u8x, u8y, "uint8"), m.distance(as_float(u8x), as_float(u8y)))


# =================================================================================================
# 6. PerceptualDistance and the transfer evaluations
# =================================================================================================
class _StubTransfer:
    """sweep(batch, rows, max_images): row r of the output is the batch scaled towards a row-dependent grey level."""

    def sweep(self, batch, rows, max_images):
        lv = torch.linspace(-0.5, 0.5, rows.shape[0], device=batch.device).view(-1, 1, 1, 1, 1)
        return (0.6 * batch.unsqueeze(0) + 0.4 * lv * torch.ones_like(batch).unsqueeze(0)).contiguous()


def test_perceptual_distance_and_class_transfer_eval():
    from wu.evaluate import ClassTransferEval, EstimatorTransferEval, PerceptualDistance
    m = _model("fp32")
    nc, b = 3, 2
    g = torch.Generator().manual_seed(4)
    batches = [(torch.rand((b, 3, 40, 33), generator=g) * 2 - 1).to(DEV) for _ in range(2)]
    tr = _StubTransfer()

    def classifier(images):
        return images.mean(dim=(2, 3))

    eye = torch.eye(nc, device=DEV)
    two, one = PerceptualDistance(m), PerceptualDistance(m)
    for bt in batches:
        two.add(bt, tr.sweep(bt, eye, 64))
    allb = torch.cat(batches)
    one.add(allb, tr.sweep(allb, eye, 64))
    r2, r1 = two.result(), one.result()
    assert r2["count"] == r1["count"] == 2 * b and r2["lpips"].shape == (nc,) and r2["lpips"].dtype == torch.float64
    # the same 2 b numbers per row, added in another order: the fp64 sum's rounding
    assert torch.all((r2["lpips"] - r1["lpips"]).abs() <= 8 * R.U * r1["lpips"].abs())
    assert abs(r2["diversity"] - r1["diversity"]) <= 8 * R.U * abs(r1["diversity"]) and r1["diversity"] > 0
    want = m.distance(allb, tr.sweep(allb, eye, 64)).mean(1).cpu()
    assert torch.all((r1["lpips"] - want).abs() <= 8 * R.U * want)
    nodiv = PerceptualDistance(m, diversity=False)
    nodiv.add(batches[0], tr.sweep(batches[0], eye, 64))
    assert nodiv.result()["diversity"] is None
    single = PerceptualDistance(m)
    single.add(batches[0], tr.sweep(batches[0], eye[:1], 64))
    assert single.result()["diversity"] is None and single.result()["lpips"].shape == (1,)

    # lpips= receives every batch; lpips=None leaves the results bit-identical
    pd = PerceptualDistance(m)
    plain, with_l = ClassTransferEval(tr, classifier, nc), ClassTransferEval(tr, classifier, nc, lpips=pd)
    for bt in batches:
        plain.update(bt)
        with_l.update(bt)
    assert torch.equal(plain.confusion(), with_l.confusion()) and int(plain.confusion().sum()) == 2 * nc * b
    res = pd.result()
    assert res["count"] == 2 * b and torch.equal(res["lpips"], r2["lpips"]) and res["diversity"] == r2["diversity"]
    pe = PerceptualDistance(m)
    ref_rows = torch.randn((2, nc), generator=g).to(DEV)
    e0, e1 = EstimatorTransferEval(tr, classifier), EstimatorTransferEval(tr, classifier, lpips=pe)
    e0.update(batches[0], ref_rows)
    e1.update(batches[0], ref_rows)
    assert torch.equal(e0.all(), e1.all()) and pe.result()["count"] == b and pe.result()["lpips"].shape == (2,)


# =================================================================================================
# 7. the command line
# =================================================================================================
def test_cli_on_two_directories(tmp_path, capsys):
    from PIL import Image
    from wu import lpips
    alex, lin = _params()
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    rng = np.random.default_rng(12)
    xs = rng.integers(0, 256, size=(4, 40, 33, 3)).astype(np.uint8)
    ys = rng.integers(0, 256, size=(4, 40, 33, 3)).astype(np.uint8)
    for i in range(4):
        Image.fromarray(xs[i]).save(a / f"im{i}.png")
        Image.fromarray(ys[i]).save(b / f"im{i}.png")
    torch.save(alex, tmp_path / "alex.pth")
    torch.save(lin, tmp_path / "lin.pth")
    assert lpips.main([str(a), str(b), "--alexnet", str(tmp_path / "alex.pth"), "--lin", str(tmp_path / "lin.pth"), "--batch-size", "3"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["LPIPS", "layers", "pairs"] and lines[-1] == "pairs: 4"
    m = _model("fp32")
    d, per = m.distance(torch.from_numpy(xs).to(DEV).permute(0, 3, 1, 2), torch.from_numpy(ys).to(DEV).permute(0, 3, 1, 2), "uint8", layers=True)
    assert abs(float(lines[0].split(":")[1]) - d.mean().item()) <= 1e-6
    got_layers = [float(v) for v in lines[1].split(":")[1].split()]
    assert len(got_layers) == 5 and np.abs(np.asarray(got_layers) - per.mean(0).cpu().numpy()).max() <= 1e-6
    with pytest.raises(SystemExit):
        lpips.main([str(a), str(b), "--lin", str(tmp_path / "lin.pth")])       # both weight arguments are required
