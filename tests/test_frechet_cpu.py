"""CPU: the numpy restatement of the rank-aware Frechet distance (tests/_frechet_ref.py, what csrc/frechet.hip computes) against LAPACK and
against scipy's sqrtm, and the round-robin schedule the kernel derives from (step, workgroup)."""
import functools
import itertools

import numpy as np
import pytest

import _frechet_ref as R


@pytest.mark.parametrize("ns", range(2, 131))
def test_schedule_meets_every_pair_once_per_sweep(ns):
    steps = R.schedule(ns)
    assert len(steps) == 2 * ((ns + 1) // 2) - 1
    seen = []
    for pairs in steps:
        assert len(pairs) in ((ns // 2,) if ns % 2 == 0 else ((ns - 1) // 2,))       # an odd ns: one vector sits each step out
        flat = [i for pq in pairs for i in pq]
        assert len(set(flat)) == len(flat), "an index appears twice in a step"
        assert all(0 <= p < q < ns for p, q in pairs)
        seen += pairs
    assert sorted(seen) == list(itertools.combinations(range(ns), 2))


def test_block_sum_is_the_sum_and_has_the_stated_order():
    rng = np.random.RandomState(0)
    for L in (1, 63, 64, 255, 256, 257, 700):
        a = rng.randint(-8, 9, (3, L)).astype(np.float64)
        assert np.array_equal(R.block_sum(a), a.sum(axis=1))               # integers: any order is exact
    # thread 0 holds 1 + 2^-53 + 2^-53 added in that order (1), thread 1 holds 2^-52: the lanes then give 1 + 2^-52
    a = np.zeros(600)
    a[0], a[256], a[512], a[1] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52
    assert R.block_sum(a) == 1.0 + 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _lapack_ratios():
    out = {}
    for name, M in R.jacobi_cases().items():
        sigma, total, rotations = R.singular_values(M)
        want = np.zeros(M.shape[0])
        sv = np.linalg.svd(M, compute_uv=False)
        want[:len(sv)] = sv
        s1 = sv[0] if sv[0] > 0 else 1.0
        got = np.sort(sigma)[::-1]
        out[name] = (np.abs(got - want).max() / ((M.shape[0] + M.shape[1]) * R.U * s1), len(rotations), sigma, total)
    return out


def test_restatement_against_lapack():
    """Over the GPU case list: max_i |sigma_i - sigma_i^svd| / ((m + n) 2^-53 sigma_1).  Measured: 0.884 at 2 x 2, 0.73 at 130 x 70, 0.67 on
    the graded matrix, 0.47 at 64 x 64, 0.34 at 63 x 70, below 0.4 elsewhere; sweeps 1 .. 27 (27 at 130 x 70, where 60 vectors have to shrink
    below the underflow floor; 16 on the graded matrix; 10 at 64 x 64).  RECORDED_WORST_RATIO holds that worst value and the GPU tolerance is
    8 x it: the device is compared with LAPACK, not with this file."""
    ratios = _lapack_ratios()
    for name, (ratio, sweeps, _, _) in ratios.items():
        print(f"{name}: ratio {ratio:.3f}, {sweeps} sweeps")
    worst = max(r[0] for r in ratios.values())
    assert worst <= R.RECORDED_WORST_RATIO, f"worst ratio {worst} over the recorded {R.RECORDED_WORST_RATIO}"
    assert R.K_GPU == 8 * R.RECORDED_WORST_RATIO


def test_restatement_special_cases():
    ratios = _lapack_ratios()
    _, sweeps, sigma, total = ratios["zero_5x9"]
    assert sweeps == 1 and np.array_equal(sigma, np.zeros(5)) and total == 0.0
    _, sweeps, sigma, _ = ratios["hadamard_16x16"]
    assert sweeps == 1 and np.array_equal(sigma, R.HADAMARD_SIGMA)            # orthogonal rows: no rotation, the norms bit for bit
    assert (ratios["130x70"][2] == 0.0).sum() >= 60                          # more vectors than length: the surplus ends at exactly zero
    assert ratios["1x5"][1] == 1
    sigma, total = ratios["63x70"][2:]
    acc = 0.0
    for v in sigma:
        acc += v
    assert total == acc                                                     # the sum in index order


def test_jacobi_raises_after_max_sweeps():
    with pytest.raises(RuntimeError, match="rotations"):
        R.jacobi(R.jacobi_cases()["64x64"], max_sweeps=1)


def _pair(n1, n2, D, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n1, D).astype(np.float32), (0.2 + 1.1 * rng.rand(n2, D) ** 2).astype(np.float32)


def _scipy_fid(x, y):
    from wu.fid import calculate_frechet_distance
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    return calculate_frechet_distance(xd.mean(axis=0), np.cov(xd, rowvar=False), yd.mean(axis=0), np.cov(yd, rowvar=False))


# D -> 100 x the relative disagreement |fid - scipy| / scipy measured on this case (n1 = 8 D, n2 = 8 D + 5, where both covariances have full
# rank and sqrtm is trustworthy): 1.2e-13 at D = 7 (fid 0.0726), 2.7e-13 at D = 16 (0.187), 1.0e-12 at D = 64 (0.789).  The two sets are
# close, so fid is a small difference of terms about D / 12 each and the relative figures are larger than each term's own error; against
# the np.linalg.svd one-liner the restatement differs by the same amounts, to two digits.
SCIPY_TOLERANCE = {7: 1.3e-11, 16: 2.8e-11, 64: 1.0e-10}


@pytest.mark.parametrize("D", sorted(SCIPY_TOLERANCE))
def test_restatement_against_scipy_where_the_covariances_have_full_rank(D):
    """D = 64 rotates 512 vectors of length 517 for 22 sweeps; it takes its dot products with einsum (kernel_order=False: the same schedule,
    threshold and rotation), which the comparison does not depend on."""
    x, y = _pair(8 * D, 8 * D + 5, D, 100 + D)
    got = R.frechet_distance(x, y, kernel_order=D < 64)
    want = _scipy_fid(x, y)
    rel = abs(got["fid"] - want) / abs(want)
    print(f"D {D}: fid {got['fid']}, scipy {want}, relative difference {rel:.3g}, {got['sweeps']} sweeps")
    assert rel <= SCIPY_TOLERANCE[D]
    assert abs(got["fid"] - R.frechet_distance_svd(x, y)) <= SCIPY_TOLERANCE[D] * abs(want)


def test_rank_deficient_case_equals_the_svd_oracle():
    """(n1, n2, D) = (40, 33, 100): both covariances have rank below D.  The restatement and the np.linalg.svd one-liner agree to 2.3e-15
    relative (measured); scipy's sqrtm of the singular product was 2.6e-8 relative away from both on the machine this was written on.  That
    offset is documented here, not asserted."""
    rng = np.random.RandomState(164)
    x, y = rng.rand(40, 100).astype(np.float32), (0.2 + 1.1 * rng.rand(33, 100) ** 2).astype(np.float32)
    got, want = R.frechet_distance(x, y), R.frechet_distance_svd(x, y)
    print(f"restatement {got['fid']}, svd {want}, scipy {_scipy_fid(x, y)}")
    # about 40 x the measured 2.3e-15: the two differ by 33 singular values' errors of up to (m + n) 2^-53 sigma_1 each and by the rounding
    # of two differently centred Gram matrices
    assert abs(got["fid"] - want) <= 1e-13 * abs(want)
    # the orientation: the 33 rows of the second set are the vectors, and swapping the sets gives the same matrix
    assert got["singular_values"].shape == (33,)
    swapped = R.frechet_distance(y, x)
    assert np.array_equal(swapped["singular_values"], got["singular_values"]) and swapped["trace1"] == got["trace2"]
