"""CPU: the definition of the radial power-spectrum metric as tests/_spectrum_ref.py restates it (the oracle of tests/test_gpu_spectrum.py),
the host-side pieces of wu.spectrum (tables, bins) against it, and ``compare`` on hand-made profiles.  No kernel is launched.

The DFT bound.  Each stage is an inner product of fp64 terms against table entries of magnitude <= 1: W terms in the row stage, 2 H in
the column stage.  With u = 2^-53, an n-term inner product computed in any order is off by at most n u sum|terms| (to first order), and the
table entries are within 1.1e-15 < 10 u of the true cosines; carried through both stages this gives, between any two correct
implementations (each off by half of it), ``|dX| <= 2 (H + W + 2) u sum|y|`` for every entry of Xr and Xi, sum|y| over the whole plane."""
import math

import numpy as np
import pytest
import torch

import _spectrum_ref as R

U = 2.0 ** -53
SHAPES = [(1, 1), (2, 2), (4, 4), (5, 7), (8, 6), (33, 17), (64, 64), (65, 96), (224, 224)]


def _planes(n, h, w, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, h, w))


@pytest.mark.parametrize("n", [1, 2, 4])
def test_small_tables_are_exact(n):
    from wu import spectrum
    for c, s in (R.twiddles(n), spectrum.twiddles(n)):
        want_c = {1: [1], 2: [1, -1], 4: [1, 0, -1, 0]}[n]
        want_s = {1: [0], 2: [0, 0], 4: [0, 1, 0, -1]}[n]
        assert c.tolist() == want_c and s.tolist() == want_s
        assert not np.signbit(s[s == 0]).any() and not np.signbit(c[c == 0]).any()


@pytest.mark.parametrize("n", [3, 5, 7, 13, 17, 23, 33, 64, 65, 96, 224])
def test_tables_against_libm_and_between_modules(n):
    from wu import spectrum
    c, s = R.twiddles(n)
    k = np.arange(n)
    assert np.abs(c - np.cos(2 * np.pi * k / n)).max() <= 1.1e-15 and np.abs(s - np.sin(2 * np.pi * k / n)).max() <= 1.1e-15
    c2, s2 = spectrum.twiddles(n)
    assert np.array_equal(c, c2) and np.array_equal(s, s2)
    assert np.array_equal(R.hann(n), spectrum.window_table(n))
    # quarter turns are exact
    for q in range(4):
        if (q * n) % 4 == 0:
            assert (c[q * n // 4], s[q * n // 4]) == ((1, 0), (0, 1), (-1, 0), (0, -1))[q]


@pytest.mark.parametrize("h,w", SHAPES + [(1, 1024), (1024, 3)])
def test_bin_counts_sum_to_the_pixel_count(h, w):
    from wu import spectrum
    idx, count, freq = R.radial_bins(h, w)
    assert int(count.sum()) == h * w and count.dtype == np.int64
    assert (count > 0).all()
    idx2, count2, freq2 = spectrum.radial_bins(h, w)
    assert idx2.dtype == np.int32 and np.array_equal(idx, idx2) and np.array_equal(count, count2) and np.array_equal(freq, freq2)
    assert freq[0] == 0 and (len(freq) == 1 or freq[1] == 1 / min(h, w))
    if (h, w) == (224, 224):
        assert count.shape[0] == 159


@pytest.mark.parametrize("n", [1, 2, 4, 5, 8, 33, 64, 224])
def test_square_rule_is_the_integer_radius(n):
    idx = R.radial_bins(n, n)[0]
    for u in range(n):
        fu = u if u <= n // 2 else u - n
        for v in range(n // 2 + 1):
            assert idx[u, v] == math.isqrt(fu * fu + v * v)


@pytest.mark.parametrize("h,w", SHAPES)
def test_half_spectrum_against_rfft2(h, w):
    y = _planes(2, h, w, 100 * h + w)
    xr, xi = R.half_spectrum(y)
    want = np.fft.rfft2(y)
    for n in range(2):
        bound = 2 * (h + w + 2) * U * np.abs(y[n]).sum()
        err = max(np.abs(xr[n] - want[n].real).max(), np.abs(xi[n] - want[n].imag).max())
        print(f"{h} x {w} image {n}: |dX| {err:.3e} against {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("window", ["none", "hann"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_parseval(h, w, window):
    x = np.random.default_rng(h * 7 + w).uniform(-1.0, 1.0, (2, 3, h, w)).astype(np.float32)
    y = R.luma(x, (-1, 1), window)
    prof, _ = R.profiles_planes(y)
    _, count, _ = R.radial_bins(h, w)
    hw = float(h * w)
    for n in range(2):
        lhs = float((prof[n] * count * (hw * hw)).sum())
        rhs = hw * float((y[n] * y[n]).sum())
        print(f"{h} x {w} {window} image {n}: {lhs:.17g} against {rhs:.17g}")
        assert abs(lhs - rhs) <= 4 * h * w * U * rhs


def test_luma_follows_the_stated_order():
    x = np.random.default_rng(3).integers(0, 256, (2, 3, 5, 7), dtype=np.uint8)
    y = R.luma(x, "uint8")
    s = x.astype(np.float64) / 255.0
    for n, i, j in ((0, 0, 0), (1, 4, 6), (1, 2, 3)):
        want = (0.299 * s[n, 0, i, j] + 0.587 * s[n, 1, i, j]) + 0.114 * s[n, 2, i, j]
        assert y[n, i, j] == want
    yh = R.luma(x, "uint8", "hann")
    assert yh[0, 0, 0] == 0.0 and yh[1, 2, 3] == (y[1, 2, 3] * R.hann(5)[2]) * R.hann(7)[3]
    one = R.luma(x[:, :1], "uint8")
    assert np.array_equal(one, s[:, 0])


# ---- compare on hand-made profiles ---------------------------------------------------------------------------------------------------------
def _bank(prof, shape=(16, 16), **kw):
    from wu import spectrum
    return spectrum.SpectrumBank(**kw).add_profiles(torch.from_numpy(np.ascontiguousarray(prof, dtype=np.float64)), shape)


def test_compare_on_hand_made_profiles():
    from wu import spectrum
    h = w = 16
    K = R.radial_bins(h, w)[1].shape[0]                # 12: bins 1 .. 8 are compared
    base = 10.0 ** (-np.arange(K) / 10.0)              # -k dB
    a = np.stack([base, base * 10.0 ** 0.2])           # two images, 2 dB apart: mean -k + 1, std 1
    gain_db = np.zeros(K)
    gain_db[1:9] = [0, 0, 1, 1, 1, -6, -2, -2]
    b = np.stack([base * 10.0 ** (gain_db / 10.0)] * 3)
    r = spectrum.compare(_bank(a), _bank(b))
    d = gain_db[1:9] - 1.0
    assert r.count_a == 2 and r.count_b == 3 and r.flat_a == 0 and r.flat_b == 0
    assert np.array_equal(r.freq, np.arange(1, 9) / 16)
    np.testing.assert_allclose(r.mean_db_a, -np.arange(1, 9) + 1.0, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r.mean_db_b, -np.arange(1, 9) + gain_db[1:9], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r.std_db_a, np.ones(8), rtol=1e-9)
    np.testing.assert_allclose(r.std_db_b, np.zeros(8), atol=1e-6)
    assert r.lsd == pytest.approx(math.sqrt(np.mean(d * d)), rel=1e-12)
    # 8 bins: thirds are [0, 2), [2, 5), [5, 8)
    assert r.bands == pytest.approx((-1.0, 0.0, -13.0 / 3.0), rel=1e-12, abs=1e-13)
    assert r.peak[0] == pytest.approx(7.0, rel=1e-12) and r.peak[1] == 6 / 16
    # and against the numpy restatement
    want = R.compare(R.bank_stats(a, 16), R.bank_stats(b, 16), 16)
    assert r.lsd == pytest.approx(want["lsd"], rel=1e-12) and r.peak[1] == want["peak"][1]
    np.testing.assert_allclose(r.bands, want["bands"], rtol=1e-12, atol=1e-13)


def test_flat_images_are_left_out():
    from wu import spectrum
    K = R.radial_bins(16, 16)[1].shape[0]
    base = 10.0 ** (-np.arange(K) / 10.0)
    black = np.zeros(K)
    holed = base.copy()
    holed[8] = 0.0                                     # a zero inside 1 .. M // 2
    beyond = base.copy()
    beyond[9:] = 0.0                                   # zeros beyond M // 2 do not make an image flat
    bank = _bank(np.stack([base, black, holed, beyond]))
    assert bank.images == 4 and bank.count == 2 and bank.flat == 2
    bank.add_profiles(torch.from_numpy(np.stack([black, base])), (16, 16))
    assert bank.images == 6 and bank.count == 3 and bank.flat == 3
    r = spectrum.compare(bank, _bank(base[None]))
    assert r.flat_a == 3 and r.count_a == 3 and r.lsd == pytest.approx(0.0, abs=1e-12)
    assert np.isfinite(r.mean_db_a).all() and np.isfinite(r.std_db_a).all()
    s1, s2, kept, flat = R.bank_stats(np.stack([base, black, holed, beyond, black, base]), 16)
    assert kept == 3 and flat == 3
    np.testing.assert_allclose(bank.sum_db[1:9].numpy(), s1[1:9], rtol=1e-12, atol=1e-13)


def test_signature_mismatch_raises():
    from wu import spectrum
    k16, k8 = R.radial_bins(16, 16)[1].shape[0], R.radial_bins(8, 8)[1].shape[0]
    a = _bank(np.ones((1, k16)))
    with pytest.raises(ValueError, match="image size"):
        spectrum.compare(a, _bank(np.ones((1, k8)), (8, 8)))
    with pytest.raises(ValueError, match="window"):
        spectrum.compare(a, _bank(np.ones((1, k16)), window="hann"))
    with pytest.raises(ValueError, match="value-range mapping"):
        spectrum.compare(a, _bank(np.ones((1, k16)), value_range="uint8"))
    with pytest.raises(ValueError, match="16 x 16"):
        a.add_profiles(torch.ones(1, k8, dtype=torch.float64), (8, 8))
    with pytest.raises(RuntimeError, match="no batch"):
        spectrum.compare(a, spectrum.SpectrumBank())
    with pytest.raises(ValueError, match="window"):
        spectrum.SpectrumBank(window="blackman")


def test_pixels_need_a_gpu_and_bad_shapes_are_named():
    from wu import spectrum
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectrum.profiles(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectrum.luma(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="1..1024"):
        spectrum.radial_bins(1025, 4)
    with pytest.raises(ValueError, match="1..1024"):
        spectrum.radial_bins(0, 4)


def test_library_ranges_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_spectrum_workspace_bytes(1, 224, 224) > 0
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 1025), (1, 1025, 8), (-1, 8, 8)):
        assert lib.wu_spectrum_workspace_bytes(n, h, w) == 0
    for h, w in SHAPES + [(1, 1024), (1024, 3), (1024, 1024), (299, 512)]:
        assert lib.wu_spectrum_bins(h, w) == R.radial_bins(h, w)[1].shape[0]
    assert lib.wu_spectrum_bins(0, 4) == 0 and lib.wu_spectrum_bins(4, 1025) == 0
    rc = lib.wu_spectrum_profiles(None, 0, 0, 0, 0, _lib.F32, 1, 2, 8, 8, 0.5, 0.5, 1.0, None, None, None, None, None, None, 7, None, None,
                                  None, None)
    assert rc < 0 and b"wu_spectrum_profiles" in lib.wu_last_error() and b"C 2" in lib.wu_last_error()
