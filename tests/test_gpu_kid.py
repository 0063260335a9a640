"""Kernel Inception Distance on the GPU (csrc/kid.hip through the C ABI and through wu.kid) against tests/_kid_ref.py.

Exact grid: integer features in {0..3}, gamma = 1/64, so every product, power and partial sum is a multiple of 2^-18 below 2^53 whatever
the order of summation -- `sums` must EQUAL the integer oracle and `mmd2` the restatement's, at the smallest legal m, across the 64-row
tile edge, with three tiles per side, with a K-chunk tail, row strides over D with poisoned padding and NaN rows behind the banks.
Real features (D = 2048, non-negative float32): |mmd2 - ref| <= 32 (D + 2) 2^-53 kbar (_kid_ref.bound: derived, not measured)."""
import functools

import numpy as np
import pytest
import torch

import _kid_ref as R
from _padded_rows import padded as _padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _exact(case):
    n1, n2, m, D, S, degree, coef0 = case
    x, y, idx = R.exact_case(case)
    want = R.exact_sums(x, y, idx, degree, R.GAMMA_DEN, coef0)
    want_mmd2 = np.array([R.mmd2_of(s[0], s[1], s[2], m) for s in want])
    return x, y, idx, want, want_mmd2


def _abi(x, y, idx, degree, gamma, coef0):
    """wu_kid_mmd called directly on contiguous uploads."""
    from wu import _lib
    lib = _lib.load()
    S, _, m = idx.shape
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    idd = torch.from_numpy(idx).to(DEV)
    nbytes = lib.wu_kid_workspace_bytes(S, m)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sums = torch.full((S, 3), NAN, dtype=torch.float64, device=DEV)
    mmd2 = torch.full((S,), NAN, dtype=torch.float64, device=DEV)
    _lib.call("wu_kid_mmd", xd.data_ptr(), xd.stride(0), x.shape[0], yd.data_ptr(), yd.stride(0), y.shape[0], idd.data_ptr(), S, m, x.shape[1],
              degree, gamma, coef0, ws.data_ptr(), sums.data_ptr(), mmd2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), mmd2.cpu().numpy()


def _assert_equal(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), \
        f"{what}: not bit-identical; max |diff| {np.nanmax(np.abs(got - want))}, got {got.reshape(-1)[:3]}, want {want.reshape(-1)[:3]}"


@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_c_abi(case):
    n1, n2, m, D, S, degree, coef0 = case
    x, y, idx, want, want_mmd2 = _exact(case)
    sums, mmd2 = _abi(x, y, idx, degree, 1.0 / R.GAMMA_DEN, float(coef0))
    _assert_equal(sums, want, "sums")
    _assert_equal(mmd2, want_mmd2, "mmd2")


@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_wu_kid_strided_and_poisoned(case):
    """Through wu.kid.polynomial_mmd_subsets, the banks as views of wider and longer buffers: ld > D with NaN padding columns, NaN rows
    after n1 / n2 (one NaN read would poison a sum)."""
    from wu import kid
    n1, n2, m, D, S, degree, coef0 = case
    x, y, idx, want, want_mmd2 = _exact(case)
    f1, f2 = _padded(x, D + 3, 2), _padded(y, D + 5, 1)
    assert f1.stride(0) == D + 3 and f2.stride(0) == D + 5
    sums, mmd2 = kid.polynomial_mmd_subsets(f1, f2, idx, degree, 1.0 / R.GAMMA_DEN, float(coef0))
    assert sums.dtype == torch.float64 and sums.shape == (S, 3) and mmd2.shape == (S,)
    _assert_equal(sums.cpu().numpy(), want, "sums")
    _assert_equal(mmd2.cpu().numpy(), want_mmd2, "mmd2")


def test_wrapper_validates_indices_on_the_host():
    from wu import kid
    x, y, idx, _, _ = _exact(R.EXACT_GRID[2])
    f1, f2 = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    for bad in (idx[:, :1], idx.astype(np.float32), idx[0]):
        with pytest.raises(ValueError, match="shape"):
            kid.polynomial_mmd_subsets(f1, f2, bad, 3, None, 1.0)
    hi, lo = idx.copy(), idx.copy()
    hi[0, 0, 0] = x.shape[0]
    lo[0, 1, 1] = -1
    for bad in (hi, lo):
        with pytest.raises(ValueError, match="outside its bank"):
            kid.polynomial_mmd_subsets(f1, f2, bad, 3, None, 1.0)
    with pytest.raises(ValueError, match="subset_size"):
        kid.polynomial_mmd_subsets(f1[:1], f2, idx[:, :, :2] * 0, 3, None, 1.0)


@functools.lru_cache(maxsize=None)
def _real(m):
    D, S = 2048, 3
    rng = np.random.RandomState(m)
    x = rng.rand(m + 11, D).astype(np.float32)
    y = (1.25 * rng.rand(m + 4, D)).astype(np.float32)
    idx = R.indices(len(x), len(y), S, m, seed=7)
    sums, mmd2 = R.subsets(x, y, idx)
    return x, y, idx, sums, mmd2, R.bound(sums, m, D)


@pytest.mark.parametrize("m", [65, 129])
def test_real_features_within_the_rounding_bound(m):
    from wu import kid
    x, y, idx, ref_sums, ref_mmd2, bound = _real(m)
    for name, (sums, mmd2) in (("abi", _abi(x, y, idx, 3, 1.0 / 2048, 1.0)),
                               ("wu.kid", [t.cpu().numpy() for t in kid.polynomial_mmd_subsets(_padded(x, 2048 + 8, 1), _padded(y, 2048, 1), idx)])):
        err = np.abs(mmd2 - ref_mmd2)
        print(f"m {m} {name}: |mmd2 - ref| {err}, bound {bound}, mmd2 {mmd2}")
        assert np.all(err <= bound), f"{name}: |mmd2 - ref| {err} over the bound {bound}"
        # the sums themselves: two evaluations of each non-negative term, 3 (D + 2) u relative each (dot product, scale and shift, two
        # multiplications), and 2 (D + 2) u more than covers summing m^2 non-negative terms pairwise or by tiles
        assert np.all(np.abs(sums - ref_sums) <= 8 * (2048 + 2) * R.U * np.abs(ref_sums))


def test_two_runs_give_identical_bits():
    x, y, idx, _, _, _ = _real(129)
    a, a2 = _abi(x, y, idx, 3, 1.0 / 2048, 1.0)
    b, b2 = _abi(x, y, idx, 3, 1.0 / 2048, 1.0)
    assert a.tobytes() == b.tobytes() and a2.tobytes() == b2.tobytes()


def test_feature_bank_ragged_batches_and_growth():
    from wu import kid
    rng = np.random.RandomState(3)
    rows = rng.rand(66, 40).astype(np.float32)
    bank = kid.FeatureBank()
    caps, at = [], 0
    for b in (1, 63, 2):
        wide = torch.full((b, 48), NAN, dtype=torch.float32, device=DEV)       # a batch with a row stride over D, as a pool3 slice has
        wide[:, :40] = torch.from_numpy(rows[at:at + b]).to(DEV)
        bank.append(wide[:, :40])
        at += b
        caps.append(bank.capacity)
        assert bank.n == at and bank.features.shape == (at, 40)
        assert np.array_equal(bank.features.cpu().numpy(), rows[:at])
    assert caps[0] == caps[1] == 64 and caps[2] == 128                         # the third batch does not fit: one doubling, rows kept
    assert bank.dim == 40 and bank.features.stride(1) == 1
    with pytest.raises(ValueError, match="differs"):
        bank.append(torch.zeros(2, 41, device=DEV))
    assert kid.FeatureBank(40).dim == 40


def test_feature_bank_npz_round_trip(tmp_path):
    from wu import kid
    rows = np.random.RandomState(4).rand(9, 12).astype(np.float32)
    bank = kid.FeatureBank()
    bank.append(torch.from_numpy(rows).to(DEV))
    path = str(tmp_path / "bank.npz")
    bank.save_npz(path)
    with np.load(path) as f:
        assert sorted(f.keys()) == ["features"] and np.array_equal(f["features"], rows)
    back = kid.FeatureBank.load_npz(path)
    assert back.n == 9 and np.array_equal(back.features.cpu().numpy(), rows)
    np.savez(str(tmp_path / "stats.npz"), mu=np.zeros(3), sigma=np.eye(3))
    with pytest.raises(ValueError, match="features"):
        kid.FeatureBank.load_npz(str(tmp_path / "stats.npz"))


def test_kernel_inception_distance_end_to_end():
    from wu import kid
    D, m, S, seed = 96, 70, 6, 5
    rng = np.random.RandomState(8)
    x = rng.rand(150, D).astype(np.float32)
    y = (rng.rand(131, D) ** 2).astype(np.float32)
    b1, b2 = kid.FeatureBank(), kid.FeatureBank()
    for lo, hi in ((0, 50), (50, 150)):
        b1.append(torch.from_numpy(x[lo:hi]).to(DEV))
    b2.append(torch.from_numpy(y).to(DEV))
    idx = kid.subset_indices(150, 131, S, m, seed)
    ref_sums, ref_mmd2 = R.subsets(x, y, idx)
    bound = R.bound(ref_sums, m, D)
    _, mmd2 = kid.polynomial_mmd_subsets(b1.features, b2.features, idx)
    err = np.abs(mmd2.cpu().numpy() - ref_mmd2)
    print(f"end to end: per-subset |mmd2 - ref| {err}, bound {bound}")
    assert np.all(err <= bound)
    mean, std = kid.kernel_inception_distance(b1, b2, num_subsets=S, subset_size=m, seed=seed)
    ref_mean, ref_std = R.kid(x, y, num_subsets=S, subset_size=m, seed=seed)
    assert isinstance(mean, float) and isinstance(std, float)
    # a mean moves by at most the largest per-subset error, and so does a standard deviation
    assert abs(mean - ref_mean) <= bound.max() and abs(std - ref_std) <= bound.max()
    assert mean > 1e-3                                                         # the two banks do differ
    with pytest.raises(ValueError, match="subset_size"):
        kid.kernel_inception_distance(b1, b2, num_subsets=S, subset_size=132)


def test_kid_of_a_bank_against_itself():
    """n = m: every subset is the whole bank in two different orders, so xx, yy and xy hold the same entries."""
    from wu import kid
    D, n, S = 64, 100, 4
    x = np.random.RandomState(9).rand(n, D).astype(np.float32)
    bank = kid.FeatureBank()
    bank.append(torch.from_numpy(x).to(DEV))
    mean, _ = kid.kernel_inception_distance(bank, bank, num_subsets=S, subset_size=n, seed=1)
    ref_mean, _ = R.kid(x, x, num_subsets=S, subset_size=n, seed=1)
    bound = R.bound(R.subsets(x, x, R.indices(n, n, S, n, 1))[0], n, D).max()
    print(f"self KID: {mean} (ref {ref_mean}), bound {bound}")
    assert abs(mean - ref_mean) <= bound


def test_statistics_of_path_also_fills_a_bank(tmp_path):
    """wu.fid.statistics_of_path(features=bank): the statistics are the ones it returns without the bank, and the bank holds the rows they
    were accumulated from, in file order over ragged batches (5, 5, 3)."""
    import _inception_ref as IRF
    import _jpeg_ref as J
    from PIL import Image
    from wu import kid
    from wu.fid import image_files, statistics_of_path
    from wu.inception import InceptionV3, global_avgpool
    from wu.layout import precision_code
    d = tmp_path / "imgs"
    d.mkdir()
    for k in range(13):
        Image.fromarray(J.synth(64, 64, 40 + k)).save(d / f"img_{k:02d}.png")
    model = InceptionV3([0])
    model.load_state_dict(IRF.make_params(True, seed=6))
    mu0, sig0 = statistics_of_path(str(d), model, 5)
    bank = kid.FeatureBank()
    mu1, sig1 = statistics_of_path(str(d), model, 5, features=bank)
    assert np.array_equal(mu0, mu1) and np.array_equal(sig0, sig1)
    rows = bank.features.cpu().numpy()
    assert rows.shape == (13, 64)
    # the rows are the network's features of the same uint8 batches, bit for bit and in file order
    files = image_files(str(d))
    want = []
    for i in range(0, 13, 5):
        batch = np.stack([np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8) for f in files[i:i + 5]])
        want.append(global_avgpool(model(torch.from_numpy(batch).to(DEV))[0], precision_code(model.precision)).cpu().numpy())
    assert np.array_equal(rows, np.concatenate(want))
    # and mu is their mean: the accumulator adds float32 differences x - shift, one rounding of at most 2^-24 |x - shift| <= 2^-23 max |x| each
    np.testing.assert_allclose(rows.astype(np.float64).mean(axis=0), mu1, rtol=0, atol=2.0 ** -23 * np.abs(rows).max())


def test_cli_prints_kid_after_fid_from_feature_npz(tmp_path, capsys):
    """`python -m wu.fid A.npz B.npz --kid`: .npz files holding `features` (one also with mu / sigma, one without) need no network."""
    from wu import fid, kid
    D, seed, S, m = 8, 3, 4, 20
    rng = np.random.RandomState(12)
    x, y = rng.rand(40, D).astype(np.float32), (0.8 * rng.rand(33, D)).astype(np.float32)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    xd = x.astype(np.float64)
    np.savez(pa, features=x, mu=xd.mean(axis=0), sigma=np.cov(xd, rowvar=False))
    bank = kid.FeatureBank()
    bank.append(torch.from_numpy(y).to(DEV))
    bank.save_npz(pb)
    argv = [pa, pb, "--weights", "unused.pth", "--kid", "--kid-subsets", str(S), "--kid-subset-size", str(m), "--kid-seed", str(seed)]
    assert fid.main(argv) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("FID: ") and lines[1].startswith("KID: ") and " ± " in lines[1]
    yd = y.astype(np.float64)
    want_fid = fid.calculate_frechet_distance(xd.mean(axis=0), np.cov(xd, rowvar=False), yd.mean(axis=0), np.cov(yd, rowvar=False))
    assert abs(float(lines[0][5:]) - want_fid) <= 1e-6 * max(1.0, abs(want_fid))
    mean, std = (float(v) for v in lines[1][5:].split(" ± "))
    idx = R.indices(40, 33, S, m, seed)
    sums, mmd2 = R.subsets(x, y, idx)
    b = R.bound(sums, m, D).max()
    assert abs(mean - np.mean(mmd2)) <= b and abs(std - np.std(mmd2)) <= b
    assert (mean, std) == fid.calculate_kid_given_paths([pa, pb], None, num_subsets=S, subset_size=m, seed=seed)
    np.savez(str(tmp_path / "c.npz"), mu=np.zeros(D), sigma=np.eye(D))
    with pytest.raises(ValueError, match="features"):
        fid.calculate_kid_given_paths([pa, str(tmp_path / "c.npz")], None, subset_size=m)
