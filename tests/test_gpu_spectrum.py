"""The radial power spectrum on the GPU (csrc/spectrum.hip through the C ABI, wu.spectrum and wu.evaluate.SpectralDiscrepancy) against
tests/_spectrum_ref.py.

* Luma: the fp64 planes EQUAL the restatement's (the same fp64 operations in the same order, no FMA).
* Exact: at (1, 1), (2, 2) and (4, 4) every table entry is 0 or +-1, so with integer planes every product and sum is an exact integer in
  any order, and the profile equals the Python-integer ground truth bit for bit after the two final divisions.
* Bounded.  With u = 2^-53: each stage is an inner product of W, respectively 2 H, fp64 terms against table entries of magnitude <= 1, so
  between any two correct implementations every entry of Xr and Xi differs by at most ``dX = 2 (H + W + 2) u sum|y|`` (sum over the
  plane; tests/test_spectrum_cpu.py holds the restatement against rfft2 with the same figure).  P = Xr Xr + Xi Xi is two products and a
  sum, three roundings: ``dP <= 2 (|Xr| + |Xi|) dX + 2 dX^2 + 3 u P``.  A bin adds at most count[k] non-negative terms (relative
  count[k] u in any order) and the quotient by count[k] and by (H W)^2 is two roundings on either side (4 u):
  ``dprof[k] <= (sum_bin weight dP) / count[k] / (H W)^2 + (count[k] + 4) u prof[k]``, everything computed from the restatement's
  values of the case.  No constant comes from a GPU run; the observed error is printed next to the bound.
* dB: ``10 log10`` moves by at most ``(10 / ln 10) r / (1 - r)`` for a relative change r, plus rtol 1e-12 for the two log implementations.

Outputs live in tests/_gpu_guard.py buffers: NaN before the call, guards on both sides checked after it."""
import functools
import math

import numpy as np
import pytest
import torch

import _spectrum_ref as R
from _gpu_guard import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}
WINDOWS = ["none", "hann"]


def _lib():
    from wu import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class GuardedF64(Guarded):
    """n doubles inside a Guarded float buffer: two NaN floats side by side are a NaN double, and the payload starts 128 bytes in."""

    def __init__(self, n):
        super().__init__(2 * n)

    def numpy(self, what, shape=None):
        out = super().numpy(what).view(np.float64)
        return out.reshape(shape) if shape is not None else out


def _dev_tables(n):
    c, s = R.twiddles(n)
    return torch.from_numpy(c).to(DEV), torch.from_numpy(s).to(DEV)


def _dev_windows(window, h, w):
    if window == "none":
        return None, None, ()
    wh, ww = torch.from_numpy(R.hann(h)).to(DEV), torch.from_numpy(R.hann(w)).to(DEV)
    return wh.data_ptr(), ww.data_ptr(), (wh, ww)


def _input_kinds(n, h, w, seed):
    """(name, CUDA tensor (N, C, H, W) of some layout, the values the kernel must see as numpy, value_range)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n, 3, h, w)).astype(np.float32)
    yield "float32 NCHW", torch.from_numpy(x).to(DEV), x, (-1, 1)
    xb = torch.from_numpy(x).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    yield "bf16 channels-last", xb, xb.float().cpu().numpy(), (-1, 1)
    u8 = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    yield "uint8 NHWC view", torch.from_numpy(u8).to(DEV).permute(0, 3, 1, 2), np.ascontiguousarray(u8.transpose(0, 3, 1, 2)), "uint8"
    big = rng.uniform(0.0, 2.0, (n, 3, h + 5, w + 9)).astype(np.float32)
    crop = torch.from_numpy(big).to(DEV)[:, :, 2:2 + h, 3:3 + w]
    assert not crop.is_contiguous() or h * w == 1
    yield "float32 crop", crop, big[:, :, 2:2 + h, 3:3 + w], (0, 2)
    g = rng.uniform(-1.0, 1.0, (n, 1, h, w)).astype(np.float32)
    yield "float32 C = 1", torch.from_numpy(g).to(DEV), g, (-1, 1)


def _abi_luma(x, value_range, window):
    L, lib = _lib()
    n, c, h, w = x.shape
    scale, shift, big_l = R.range_mapping(value_range)
    out = GuardedF64(n * h * w)
    ph, pw, _keep = _dev_windows(window, h, w)
    L.call("wu_spectrum_luma", x.data_ptr(), *x.stride(), CODES[x.dtype], n, c, h, w, scale, shift, big_l, ph, pw, out.ptr, _stream())
    torch.cuda.synchronize()
    return out.numpy("wu_spectrum_luma", (n, h, w))


def _abi_planes(y, want_sum=False):
    """(prof (N, K), spectrum sum (H, Wh) or None) of host planes (N, H, W) through wu_spectrum_profiles_planes."""
    L, lib = _lib()
    n, h, w = y.shape
    K = lib.wu_spectrum_bins(h, w)
    nbytes = lib.wu_spectrum_workspace_bytes(n, h, w)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    yd = torch.from_numpy(np.array(y, dtype=np.float64)).to(DEV)
    cw, sw = _dev_tables(w)
    ch, sh = _dev_tables(h)
    prof = GuardedF64(n * K)
    total = None
    if want_sum:
        total = GuardedF64(h * (w // 2 + 1))
        total.view.zero_()
    L.call("wu_spectrum_profiles_planes", yd.data_ptr(), n, h, w, cw.data_ptr(), sw.data_ptr(), ch.data_ptr(), sh.data_ptr(), K,
           ws.data_ptr(), prof.ptr, total.ptr if want_sum else None, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y), "wu_spectrum_profiles_planes: input modified"
    return prof.numpy("wu_spectrum_profiles_planes", (n, K)), total.numpy("spectrum sum", (h, w // 2 + 1)) if want_sum else None


def _abi_fused(x, value_range, window):
    L, lib = _lib()
    n, c, h, w = x.shape
    scale, shift, big_l = R.range_mapping(value_range)
    K = lib.wu_spectrum_bins(h, w)
    ws = torch.full((lib.wu_spectrum_workspace_bytes(n, h, w),), 0xFF, dtype=torch.uint8, device=DEV)
    cw, sw = _dev_tables(w)
    ch, sh = _dev_tables(h)
    ph, pw, _keep = _dev_windows(window, h, w)
    prof = GuardedF64(n * K)
    L.call("wu_spectrum_profiles", x.data_ptr(), *x.stride(), CODES[x.dtype], n, c, h, w, scale, shift, big_l, ph, pw, cw.data_ptr(),
           sw.data_ptr(), ch.data_ptr(), sh.data_ptr(), K, ws.data_ptr(), prof.ptr, None, _stream())
    torch.cuda.synchronize()
    return prof.numpy("wu_spectrum_profiles", (n, K))


def _bounds(y, xr, xi):
    """(dP (N, H, Wh), dprof (N, K)) of the module docstring for planes y and (exact or restated) Xr, Xi."""
    n, h, w = y.shape
    idx, count, _ = R.radial_bins(h, w)
    weight = R.mirror_weights(w).astype(np.float64)
    dx = (2 * (h + w + 2) * U * np.abs(y).sum((1, 2)))[:, None, None]
    p = xr * xr + xi * xi
    dp = 2 * (np.abs(xr) + np.abs(xi)) * dx + 2 * dx * dx + 3 * U * p
    hw2 = float(h * w) ** 2
    K = count.shape[0]
    cnt = count.astype(np.float64)
    sum_dp = np.stack([np.bincount(idx.reshape(-1), (dp[i] * weight).reshape(-1), K) for i in range(n)])
    prof = np.stack([np.bincount(idx.reshape(-1), (p[i] * weight).reshape(-1), K) for i in range(n)]) / cnt / hw2
    return dp, sum_dp / cnt / hw2 + (cnt + 4) * U * prof


@functools.lru_cache(maxsize=None)
def _reference(h, w, n, seed):
    y = np.random.default_rng(seed).uniform(0.0, 1.0, (n, h, w))
    xr, xi = R.half_spectrum(y)
    prof, p = R.profiles_planes(y)
    for a in (y, xr, xi, prof, p):
        a.setflags(write=False)
    return y, xr, xi, prof, p


# ---------------------------------------------------------------------------------------------------------------------------------
# luma
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 17), (64, 64), (65, 96)])
def test_luma_is_bit_equal(h, w, window):
    from wu import spectrum
    for name, x, seen, value_range in _input_kinds(2, h, w, 10 * h + w):
        want = R.luma(seen, value_range, window)
        got = _abi_luma(x, value_range, window)
        assert np.array_equal(got, want), f"{name} {h} x {w} {window}"
        assert np.array_equal(spectrum.luma(x, value_range, window).cpu().numpy(), want), f"wu.spectrum.luma, {name}"


# ---------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------
def _integer_profile(y):
    """The profile of one integer plane (H, W), H = W in {1, 2, 4}, with Python integers up to the two final divisions."""
    h, w = y.shape
    unit = {1: [(1, 0)], 2: [(1, 0), (-1, 0)], 4: [(1, 0), (0, 1), (-1, 0), (0, -1)]}
    idx, count, _ = R.radial_bins(h, w)
    sums = [0] * count.shape[0]
    for u in range(h):
        for v in range(w // 2 + 1):
            xr = xi = 0
            for i in range(h):
                for j in range(w):
                    c1, s1 = unit[h][(u * i) % h]
                    c2, s2 = unit[w][(v * j) % w]
                    c, s = c1 * c2 - s1 * s2, s1 * c2 + c1 * s2          # e^{-i a}: (c, -s)
                    xr += int(y[i, j]) * c
                    xi -= int(y[i, j]) * s
            sums[idx[u, v]] += (2 if 0 < 2 * v < w else 1) * (xr * xr + xi * xi)
    return [float(s) / float(c) / float((h * w) ** 2) for s, c in zip(sums, count.tolist())]


@pytest.mark.parametrize("n", [1, 2, 4])
def test_integer_planes_are_exact(n):
    y = np.random.default_rng(n).integers(0, 256, (5, n, n)).astype(np.float64)
    y[0] = 255.0
    got, _ = _abi_planes(y)
    want = np.array([_integer_profile(y[i]) for i in range(y.shape[0])])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, R.profiles_planes(y)[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# bounded
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (8, 6), (33, 17), (64, 64), (65, 96), (1, 1024), (1024, 3), (224, 224)])
def test_profiles_within_the_derived_bound(h, w):
    y, xr, xi, want, p = _reference(h, w, 2, 1000 * h + w)
    got, total = _abi_planes(y, want_sum=True)
    dp, bound = _bounds(y, xr, xi)
    err = np.abs(got - want)
    print(f"{h} x {w}: profile error / bound, worst bin {np.max(err / bound):.3e}; largest error {err.max():.3e}, its bound "
          f"{bound.reshape(-1)[err.argmax()]:.3e}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (err <= bound).all()
    # the running spectrum sum: P of both images, each within dP, added in ascending n (one more rounding)
    sum_want = p[0] + p[1]
    sum_bound = dp[0] + dp[1] + 2 * U * sum_want
    sum_err = np.abs(total - sum_want)
    print(f"{h} x {w}: spectrum-sum error / bound, worst entry {np.max(sum_err / sum_bound):.3e}")
    assert (sum_err <= sum_bound).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# fused = two-step
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("h,w", [(33, 17), (65, 96)])
def test_fused_equals_luma_then_planes(h, w, window):
    from wu import spectrum
    for name, x, seen, value_range in _input_kinds(3, h, w, 7 * h + w):
        planes = _abi_luma(x, value_range, window)
        two_step, _ = _abi_planes(planes)
        fused = _abi_fused(x, value_range, window)
        assert np.array_equal(fused, two_step), f"{name} {h} x {w} {window}"
        assert np.array_equal(spectrum.profiles(x, value_range, window).cpu().numpy(), fused), f"wu.spectrum.profiles, {name}"
        assert np.array_equal(spectrum.profiles_planes(torch.from_numpy(planes).to(DEV)).cpu().numpy(), fused)


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism and chunking
# ---------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_across_runs_and_chunkings():
    from wu import spectrum
    h, w = 33, 17
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, (5, 3, h, w)).astype(np.float32)).to(DEV)
    seen = []
    for max_images in (1, 2, 5, 1, 2, 5, None):
        total = torch.zeros(h, w // 2 + 1, dtype=torch.float64, device=DEV)
        prof = spectrum.profiles(x, window="hann", max_images=max_images, mean_spectrum=total)
        seen.append((prof.cpu().numpy().tobytes(), total.cpu().numpy().tobytes()))
        assert np.array_equal(spectrum.profiles(x, window="hann", max_images=max_images).cpu().numpy(), prof.cpu().numpy())
    assert all(s == seen[0] for s in seen)
    # an image's profile does not depend on its neighbours in the batch
    alone = spectrum.profiles(x[3:4], window="hann")
    assert alone.cpu().numpy().tobytes() == spectrum.profiles(x, window="hann")[3:4].cpu().numpy().tobytes()


def test_the_largest_call_and_the_chunk_after_it():
    """65 535 images is the most one library call takes (the column stage's grid.y); 65 540 one-pixel images go through as two chunks,
    and the profile of a one-pixel image is its value squared, exactly."""
    from wu import spectrum
    v = np.random.default_rng(8).uniform(0.0, 1.0, (65540, 1, 1, 1)).astype(np.float32)
    assert spectrum.default_max_images(1, 1) == spectrum.MAX_IMAGES == 65535
    got = spectrum.profiles(torch.from_numpy(v).to(DEV), value_range=(0, 1)).cpu().numpy()
    want = v.astype(np.float64).reshape(-1, 1) ** 2
    assert got.shape == (65540, 1) and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# property
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(32, 32), (40, 24)])
def test_a_cosine_lands_in_its_bin(h, w):
    f = 5
    y = np.broadcast_to(np.cos(2 * np.pi * f * np.arange(w) / w), (1, h, w)).copy()
    got, _ = _abi_planes(y)
    idx, count, _ = R.radial_bins(h, w)
    xr = np.zeros((1, h, w // 2 + 1))
    xr[0, 0, f] = h * w / 2                       # the exact transform of the exact cosine
    _, bound = _bounds(y, xr, np.zeros_like(xr))
    k = int(idx[0, f])
    want = np.zeros_like(got)
    want[0, k] = 0.25 * 2 / count[k]
    err = np.abs(got - want)
    print(f"{h} x {w}: bin {k} value {got[0, k]:.17g} against {want[0, k]:.17g}, error / bound worst bin {np.max(err / bound):.3e}")
    assert int(np.argmax(got[0])) == k
    assert (err <= bound).all()


@pytest.mark.parametrize("h,w", [(32, 32), (40, 24)])
def test_a_constant_plane_is_all_in_bin_zero(h, w):
    y = np.full((1, h, w), 0.5)
    got, _ = _abi_planes(y)
    xr = np.zeros((1, h, w // 2 + 1))
    xr[0, 0, 0] = 0.5 * h * w
    _, bound = _bounds(y, xr, np.zeros_like(xr))
    want = np.zeros_like(got)
    want[0, 0] = 0.25 / R.radial_bins(h, w)[1][0]          # bin 0 may hold more than the DC entry (40 x 24: fu = +-1 too)
    assert (np.abs(got - want) <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sets():
    """Two seeded sets of 6 and 9 images at 32 x 32 (the last of the 9 is black), their restated profiles and dB bounds."""
    rng = np.random.default_rng(11)
    a = rng.uniform(-1.0, 1.0, (6, 3, 32, 32)).astype(np.float32)
    b = (0.7 * rng.uniform(-1.0, 1.0, (9, 3, 32, 32))).astype(np.float32)
    b[:, :, :, ::2] *= 0.5                        # a periodic mark, so that the two sides differ
    b[8] = -1.0
    out = []
    for x in (a, b):
        y = R.luma(x)
        xr, xi = R.half_spectrum(y)
        prof, _ = R.profiles_planes(y)
        _, bound = _bounds(y, xr, xi)
        out.append((x, prof, bound))
    return out


def _db_bound(prof, bound):
    """Per bin of 1 .. 16: how far the mean dB of the kept images of a side may be from the restatement's."""
    flat = np.any(prof[:, 1:17] == 0.0, axis=1)
    prof, bound = prof[~flat, 1:17], bound[~flat, 1:17]
    rel = bound / prof
    assert (rel < 1e-6).all()
    each = 10.0 / math.log(10.0) * rel / (1.0 - rel) + 1e-12 * np.abs(10.0 * np.log10(prof))
    return each.mean(0), float(np.abs(10.0 * np.log10(prof)).max())


def _check_result(r, rows_a, rows_b, what):
    """r against the restatement for the images rows_a of set a / rows_b of set b (index arrays; a side may come from either set)."""
    (set_a, ia), (set_b, ib) = rows_a, rows_b
    sets = _sets()
    pa, ba = sets[set_a][1][ia], sets[set_a][2][ia]
    pb, bb = sets[set_b][1][ib], sets[set_b][2][ib]
    want = R.compare(R.bank_stats(pa, 32), R.bank_stats(pb, 32), 32)
    ea, big_a = _db_bound(pa, ba)
    eb, big_b = _db_bound(pb, bb)
    assert np.array_equal(r.freq, want["freq"])
    for tag, err, big, stats in (("a", ea, big_a, R.bank_stats(pa, 32)), ("b", eb, big_b, R.bank_stats(pb, 32))):
        got = getattr(r, "mean_db_" + tag)
        print(f"{what}: mean dB {tag}, error / bound worst bin {np.max(np.abs(got - want['mean_db_' + tag]) / err):.3e}")
        assert (np.abs(got - want["mean_db_" + tag]) <= err).all()
        # var = mean(dB^2) - mean^2: each term moves by at most 2 max|dB| err + err^2, and carries 1e-12 of max|dB|^2 of log and sum noise
        var_bound = 2 * (2 * big * err + err * err) + 4e-12 * big * big
        got_var, want_var = getattr(r, "std_db_" + tag) ** 2, want["std_db_" + tag] ** 2
        assert (np.abs(got_var - want_var) <= var_bound).all()
        assert (getattr(r, "count_" + tag), getattr(r, "flat_" + tag)) == (stats[2], stats[3])
    e = ea + eb
    assert abs(r.lsd - want["lsd"]) <= e.max()
    assert np.abs(np.array(r.bands) - np.array(want["bands"])).max() <= e.max()
    assert abs(r.peak[0] - want["peak"][0]) <= e.max() and r.peak[1] == want["peak"][1]


def test_banks_and_compare_end_to_end():
    from wu import spectrum
    (a, _, _), (b, _, _) = _sets()
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    bank_a = spectrum.SpectrumBank().add(ta[:4]).add(ta[4:])
    bank_b = spectrum.SpectrumBank(keep_mean_spectrum=True).add(tb[:2]).add(tb[2:])
    assert (bank_a.count, bank_a.flat, bank_b.count, bank_b.flat) == (6, 0, 8, 1)
    r = spectrum.compare(bank_a, bank_b)
    _check_result(r, (0, np.arange(6)), (1, np.arange(9)), "compare")
    assert r.lsd > 0.1                             # the two sets do differ
    one = spectrum.SpectrumBank(keep_mean_spectrum=True).add(tb)
    assert np.array_equal(one.mean_spectrum().cpu().numpy(), bank_b.mean_spectrum().cpu().numpy())
    with pytest.raises(ValueError, match="window"):
        spectrum.compare(bank_a, spectrum.SpectrumBank(window="hann").add(tb))
    pic = spectrum.spectrum_picture(one.mean_spectrum(), bank_b.mean_spectrum(), 32)
    assert tuple(pic.shape) == (32, 68, 3) and pic.dtype == torch.uint8
    assert torch.equal(pic[:, :32], pic[:, 36:]) and int(pic[16, 16, 0]) == 255      # DC in the middle after the shift


def test_spectral_discrepancy_rows_and_reference():
    from wu import spectrum
    from wu.evaluate import SpectralDiscrepancy
    (a, _, _), (b, _, _) = _sets()
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    rows = [np.arange(0, 6), np.arange(3, 9)]
    fake = torch.stack([tb[0:6], tb[3:9]])
    acc = SpectralDiscrepancy()
    acc.update(ta[:3], fake[:, :3])
    acc.update(ta[3:], fake[:, 3:])
    out = acc.compute()
    assert isinstance(out, list) and len(out) == 2
    for r, idx in zip(out, rows):
        _check_result(r, (0, np.arange(6)), (1, idx), "SpectralDiscrepancy rows")
    assert (out[0].flat_b, out[1].flat_b) == (0, 1)
    single = SpectralDiscrepancy()
    single.update(ta, tb[:6])
    _check_result(single.compute(), (0, np.arange(6)), (1, np.arange(6)), "SpectralDiscrepancy")
    ref = spectrum.SpectrumBank().add(tb)
    acc = SpectralDiscrepancy(reference=ref)
    acc.update(tb[:6], torch.stack([ta, tb[3:9]]))
    out = acc.compute()
    _check_result(out[0], (1, np.arange(9)), (0, np.arange(6)), "reference=, row 0")
    _check_result(out[1], (1, np.arange(9)), (1, rows[1]), "reference=, row 1")
    with pytest.raises(ValueError, match="window"):
        bad = SpectralDiscrepancy(window="hann", reference=ref)
        bad.update(ta, ta)
        bad.compute()


def test_transfer_evaluations_hand_every_batch_to_spectrum():
    """spectrum= changes nothing in what the evaluations computed before, and the accumulator has seen (batch, sweep output) of every
    update: its banks equal banks filled by hand, bit for bit."""
    import cunet
    from wu import spectrum
    from wu.evaluate import ClassTransferEval, EstimatorTransferEval, SpectralDiscrepancy
    from wu.train_step import StandInEstimator
    nc, b = 5, 3
    torch.manual_seed(0)
    net = cunet.Conditional_UNet(nc, precision="bf16").to(DEV).eval()
    torch.manual_seed(11)
    est = StandInEstimator(nc).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand((b, 3, 64, 64), generator=g) * 2 - 1).to(DEV) for _ in range(2)]
    ref_rows = torch.randn((2, nc), generator=g).to(DEV)
    acc = SpectralDiscrepancy(window="hann")
    plain, with_s = ClassTransferEval(net, est, nc), ClassTransferEval(net, est, nc, spectrum=acc)
    real = spectrum.SpectrumBank(window="hann")
    rows = [spectrum.SpectrumBank(window="hann") for _ in range(nc)]
    with torch.no_grad():
        for batch in batches:
            plain.update(batch)
            with_s.update(batch)
            fakes = net.sweep(batch, torch.eye(nc, device=DEV), with_s.max_images)
            real.add(batch)
            for bank, f in zip(rows, fakes):
                bank.add(f)
    assert torch.equal(plain.confusion(), with_s.confusion())
    out = acc.compute()
    assert len(out) == nc and all(r.count_a == 2 * b and r.count_b == 2 * b for r in out)
    for r, bank in zip(out, rows):
        want = spectrum.compare(real, bank)
        assert r.lsd == want.lsd and r.bands == want.bands and r.peak == want.peak and np.array_equal(r.mean_db_b, want.mean_db_b)
        assert np.isfinite(r.lsd) and len(r.freq) == 32
    a2 = SpectralDiscrepancy()
    e0, e1 = EstimatorTransferEval(net, est), EstimatorTransferEval(net, est, spectrum=a2)
    with torch.no_grad():
        e0.update(batches[0], ref_rows)
        e1.update(batches[0], ref_rows)
    assert torch.equal(e0.all(), e1.all())
    assert len(a2.compute()) == 2 and a2.compute()[0].count_b == b


# ---------------------------------------------------------------------------------------------------------------------------------
# directories and the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def _hand_bank(files, size=None, filter=None, batch_size=64, **kw):
    """A bank filled batch by batch from wu.files.read_images, the way a caller without from_dir would."""
    from wu import spectrum
    from wu.files import read_images
    bank = spectrum.SpectrumBank(**kw)
    for x, value_range in read_images(files, size, False, DEV, batch_size, filter=filter):
        bank.value_range = value_range
        bank.add(x)
    return bank


def test_command_line(tmp_path, capsys):
    """python -m wu.spectrum on two small directories (PNG and JPEG files, 5 against 7 images): the printed line and the --json contents
    are compare() of banks filled by hand, without and with --window hann and --size / --filter; --mean-spectrum writes the picture of
    spectrum_picture as a decodable PNG of shape (H, 2 W + 4); mixed sizes without --size raise."""
    import json
    from PIL import Image
    from wu import spectrum
    from wu.files import image_files
    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, (5, 32, 40, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (7, 32, 40, 3)).astype(np.float64)
    b = ((b + np.roll(b, 1, 1) + np.roll(b, 1, 2)) / 3).astype(np.uint8)          # blurred: the upper band must come out negative
    for name, arr in (("a", a), ("b", b)):
        (tmp_path / name).mkdir()
        for i, img in enumerate(arr):
            if name == "b" and i == 2:
                Image.fromarray(img).save(tmp_path / name / f"{i:02d}.jpg", quality=90)
            else:
                Image.fromarray(img).save(tmp_path / name / f"{i:02d}.png")
    da, db = str(tmp_path / "a"), str(tmp_path / "b")
    fa, fb = image_files(da), image_files(db)
    assert (len(fa), len(fb)) == (5, 7)
    # the pixels as Pillow reads them, in the listing's order: uint8 NHWC storage seen as NCHW, value range "uint8"
    xa, xb = (torch.from_numpy(np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])).to(DEV).permute(0, 3, 1, 2)
              for files in (fa, fb))
    for window in WINDOWS:
        jp = tmp_path / f"{window}.json"
        assert spectrum.main([da, db, "--json", str(jp)] + (["--window", "hann"] if window == "hann" else [])) == 0
        out = capsys.readouterr().out
        want = spectrum.compare(spectrum.SpectrumBank("uint8", window).add(xa), spectrum.SpectrumBank("uint8", window).add(xb))
        lines = [ln for ln in out.splitlines() if ln.startswith("Spectrum:")]
        assert lines == [spectrum.format_line(want)]
        assert "images 5 against 7" in lines[0] and "flat 0 / 0" in lines[0] and want.bands[2] < -1.0
        d = json.loads(jp.read_text())
        assert d["freq"] == want.freq.tolist() and len(d["freq"]) == 16 and d["image size"] == [32, 40] and d["window"] == window
        for key in ("mean_db_a", "mean_db_b", "std_db_a", "std_db_b"):
            assert d[key] == getattr(want, key).tolist(), key
        assert (d["lsd"], tuple(d["bands"]), tuple(d["peak"])) == (want.lsd, want.bands, want.peak)
        assert (d["count_a"], d["count_b"], d["flat_a"], d["flat_b"]) == (5, 7, 0, 0)
    # the mean-spectrum picture, through the PNG encoder of the drivers
    pp = tmp_path / "mean.png"
    assert spectrum.main([da, db, "--mean-spectrum", str(pp)]) == 0
    capsys.readouterr()
    banks = [spectrum.SpectrumBank("uint8", keep_mean_spectrum=True).add(x) for x in (xa, xb)]
    pic = np.asarray(Image.open(pp))
    assert pic.shape == (32, 2 * 40 + 4, 3) and pic.dtype == np.uint8
    assert np.array_equal(pic, spectrum.spectrum_picture(banks[0].mean_spectrum(), banks[1].mean_spectrum(), 40).cpu().numpy())
    assert pic[16, 20, 0] == 255 and not pic[:, 40:44].any()                       # DC of side a in its middle; the black gap
    # from_dir is the bank of the directory
    got = spectrum.SpectrumBank.from_dir(db, batch_size=3, window="hann")
    one = spectrum.SpectrumBank("uint8", "hann").add(xb)
    assert got.signature() == one.signature() and got.images == 7
    assert np.array_equal(got.sum_db.cpu().numpy(), _hand_bank(fb, batch_size=3, window="hann").sum_db.cpu().numpy())
    # mixed sizes: an error without --size, one size with it (the float range of the resizers)
    Image.fromarray(rng.integers(0, 256, (44, 36, 3), dtype=np.uint8)).save(tmp_path / "a" / "99.png")
    with pytest.raises(ValueError, match="--size"):
        spectrum.main([da, db])
    capsys.readouterr()
    fa = image_files(da)
    for extra, kw in (([], {}), (["--filter", "bicubic", "--window", "hann"], {"filter": "bicubic"})):
        assert spectrum.main([da, db, "--size", "24"] + extra) == 0
        out = capsys.readouterr().out
        window = "hann" if extra else "none"
        want = spectrum.compare(_hand_bank(fa, 24, window=window, **kw), _hand_bank(fb, 24, window=window, **kw))
        assert [ln for ln in out.splitlines() if ln.startswith("Spectrum:")] == [spectrum.format_line(want)]
        assert "images 6 against 7" in out and len(want.freq) == 12
    with pytest.raises(SystemExit):
        spectrum.main([da, db, "--filter", "bicubic"])
    capsys.readouterr()
    with pytest.raises(RuntimeError, match="no .jpg / .png"):
        (tmp_path / "empty").mkdir()
        spectrum.main([da, str(tmp_path / "empty"), "--size", "24"])


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched():
    from wu import spectrum
    L, lib = _lib()
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    cw, sw = _dev_tables(8)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    for n, c, h, w, name in ((1, 2, 8, 8, b"C 2"), (1, 3, 0, 8, b"out of range"), (1, 3, 8, 1025, b"out of range"), (0, 3, 8, 8, b"out of range")):
        out = GuardedF64(4096)
        rc = lib.wu_spectrum_luma(x.data_ptr(), *x.stride(), 0, n, c, h, w, 0.5, 0.5, 1.0, None, None, out.ptr, _stream())
        assert rc != 0 and b"wu_spectrum_luma" in lib.wu_last_error() and name in lib.wu_last_error()
        rc = lib.wu_spectrum_profiles(x.data_ptr(), *x.stride(), 0, n, c, h, w, 0.5, 0.5, 1.0, None, None, cw.data_ptr(), sw.data_ptr(),
                                      cw.data_ptr(), sw.data_ptr(), 6, ws.data_ptr(), out.ptr, None, _stream())
        assert rc != 0 and b"wu_spectrum_profiles" in lib.wu_last_error() and name in lib.wu_last_error()
        if c == 3:
            rc = lib.wu_spectrum_profiles_planes(out.ptr, n, h, w, cw.data_ptr(), sw.data_ptr(), cw.data_ptr(), sw.data_ptr(), 6, ws.data_ptr(),
                                                 out.ptr, None, _stream())
            assert rc != 0 and b"wu_spectrum_profiles_planes" in lib.wu_last_error()
            assert lib.wu_spectrum_workspace_bytes(n, h, w) == 0
        torch.cuda.synchronize()
        out.untouched("a rejected wu_spectrum call")
    assert lib.wu_spectrum_workspace_bytes(65535, 8, 8) > 0 and lib.wu_spectrum_workspace_bytes(65536, 8, 8) == 0
    out = GuardedF64(64)
    rc = lib.wu_spectrum_profiles(x.data_ptr(), *x.stride(), 0, 1, 3, 8, 8, 0.5, 0.5, 1.0, None, None, cw.data_ptr(), sw.data_ptr(),
                                  cw.data_ptr(), sw.data_ptr(), 5, ws.data_ptr(), out.ptr, None, _stream())
    assert rc != 0 and b"radial bins" in lib.wu_last_error()                       # 8 x 8 has 6
    rc = lib.wu_spectrum_luma(x.data_ptr(), *x.stride(), 7, 1, 3, 8, 8, 0.5, 0.5, 1.0, None, None, out.ptr, _stream())
    assert rc != 0 and b"dtype" in lib.wu_last_error()
    torch.cuda.synchronize()
    out.untouched("a rejected wu_spectrum call")
    for bad, match in ((torch.zeros(1, 2, 8, 8, device=DEV), "C 1 or 3"), (torch.zeros(1, 3, 8, 1025, device=DEV), "1..1024"),
                       (torch.zeros(1, 3, 8, 8, device=DEV, dtype=torch.float16), "float32, bfloat16 or uint8")):
        with pytest.raises(ValueError, match=match):
            spectrum.profiles(bad)
        with pytest.raises(ValueError, match=match):
            spectrum.luma(bad)
    with pytest.raises(ValueError, match="window"):
        spectrum.profiles(x, window="blackman")
