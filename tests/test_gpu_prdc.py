"""Improved precision / recall and density / coverage on the GPU (csrc/prdc.hip through the C ABI and through wu.prdc) against
tests/_prdc_ref.py.

Exact grid: integer features in {0..3}, so every d^2 is an exact integer in fp64 whatever the order of summation -- radii, A, B and C must
EQUAL the int64 oracle, at the smallest legal shape, at n = k + 1, across the 64-row tile edge, with a K-chunk tail, duplicate rows (radius
0), three tiles per side and k = 16, for col_splits 0 (the library's choice), 1, 2 and 3 (a split of whole tiles, a ragged one, an empty
one), on contiguous uploads and on views of wider, longer NaN-filled buffers.  The cases hold 4 - 195 pairs with d^2 == radius, so `<=`
against `<` is decided here (tests/test_prdc_cpu.py checks that they do).
Real features (D = 2048): no reference comparison lies within the rounding bound 4 (D + 2) 2^-53 (max|x|^2 + max|y|^2) of its radius
(_prdc_ref.bound: derived, not measured; checked here, a violation fails), so the counts must equal the reference's and the radii lie
within the bound."""
import functools

import numpy as np
import pytest
import torch

import _prdc_ref as R
from _padded_rows import padded as _padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _exact(case):
    x, y = R.exact_case(case)
    return x, y, R.exact(x, y, case[3])


@functools.lru_cache(maxsize=None)
def _real(case):
    x, y = R.real_case(case)
    return x, y, R.real(x, y, case[2]), R.bound(x, y, R.REAL_D)


def _abi(x, y, k, col_splits):
    """wu_knn_radii on each bank, then wu_prdc_counts, called directly on contiguous uploads; the outputs start poisoned."""
    from wu import _lib
    lib = _lib.load()
    (n1, D), n2 = x.shape, y.shape[0]
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    nbytes = lib.wu_prdc_workspace_bytes(n1, n2, k, col_splits)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)          # NaN doubles
    rx = torch.full((n1,), NAN, dtype=torch.float64, device=DEV)
    ry = torch.full((n2,), NAN, dtype=torch.float64, device=DEV)
    A, B, C = (torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device=DEV) for n in (n1, n1, n2))
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("wu_knn_radii", xd.data_ptr(), xd.stride(0), n1, D, k, col_splits, ws.data_ptr(), rx.data_ptr(), stream)
    _lib.call("wu_knn_radii", yd.data_ptr(), yd.stride(0), n2, D, k, col_splits, ws.data_ptr(), ry.data_ptr(), stream)
    _lib.call("wu_prdc_counts", xd.data_ptr(), xd.stride(0), n1, rx.data_ptr(), yd.data_ptr(), yd.stride(0), n2, ry.data_ptr(), D,
              ws.data_ptr(), A.data_ptr(), B.data_ptr(), C.data_ptr(), stream)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (A, B, C, rx, ry))


def _assert_counts(got, ref, what):
    for name, g, w in zip("ABC", got[:3], (ref.A, ref.B, ref.C)):
        bad = np.flatnonzero(g.astype(np.int64) != w)
        assert g.shape == w.shape and bad.size == 0, f"{what}: {name} differs at {bad[:8]}: got {g[bad[:8]]}, want {w[bad[:8]]}"
    assert int(got[0].sum()) == int(got[2].sum())


def _assert_exact(got, ref, what):
    for name, g, w in (("radii_x", got[3], ref.radii_x), ("radii_y", got[4], ref.radii_y)):
        bad = np.flatnonzero(g != w.astype(np.float64))
        assert g.dtype == np.float64 and g.shape == w.shape and bad.size == 0, \
            f"{what}: {name} differs at {bad[:8]}: got {g[bad[:8]]}, want {w[bad[:8]]}"
    _assert_counts(got, ref, what)


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_c_abi(case, col_splits):
    x, y, ref = _exact(case)
    _assert_exact(_abi(x, y, case[3], col_splits), ref, f"abi splits {col_splits}")


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_wu_prdc_strided_and_poisoned(case, col_splits):
    """Through wu.prdc, the banks as views of wider and longer buffers: ld > D with NaN padding columns, NaN rows after n1 / n2 (one NaN
    read into a result would change a radius or a count)."""
    from wu import prdc
    n1, n2, D, k = case
    x, y, ref = _exact(case)
    f1, f2 = _padded(x, D + 3, 2), _padded(y, D + 5, 1)
    assert f1.stride(0) == D + 3 and f2.stride(0) == D + 5
    out = prdc.manifold_counts(f1, f2, k, col_splits)
    assert [t.dtype for t in out] == [torch.int32] * 3 + [torch.float64] * 2 and [len(t) for t in out] == [n1, n1, n2, n1, n2]
    _assert_exact(tuple(t.cpu().numpy() for t in out), ref, f"wu.prdc splits {col_splits}")
    assert np.array_equal(prdc.knn_radii(f2, k, col_splits).cpu().numpy(), ref.radii_y.astype(np.float64))
    if col_splits == 0:
        assert prdc.precision_recall_density_coverage(f1, f2, k) == R.metrics(ref.A, ref.B, ref.C, k)


@pytest.mark.parametrize("case", R.REAL_CASES, ids=lambda c: "n%dx%d_k%d" % c)
def test_real_features_counts_equal_and_radii_within_the_bound(case):
    from wu import prdc
    n1, n2, k = case
    x, y, ref, bound = _real(case)
    # the conditions under which the counts must be equal: checked, never skipped
    margin = R.smallest_margin(ref)
    assert margin > bound, f"a reference pair lies within the bound {bound} of its radius (margin {margin})"
    for v in (ref.A, ref.C):
        assert (v == 0).any() and (v > 0).any()
    runs = (("abi", _abi(x, y, k, 0)), ("abi splits 2", _abi(x, y, k, 2)),
            ("wu.prdc", tuple(t.cpu().numpy() for t in prdc.manifold_counts(_padded(x, R.REAL_D + 8, 1), _padded(y, R.REAL_D, 1), k))))
    for name, got in runs:
        ex = np.abs(got[3] - ref.radii_x).astype(np.float64).max()
        ey = np.abs(got[4] - ref.radii_y).astype(np.float64).max()
        print(f"{case} {name}: max |radii - ref| {ex:.3e} / {ey:.3e}, bound {bound:.3e}, smallest margin {margin:.3e}, "
              f"metrics {R.metrics(*[g.astype(np.int64) for g in got[:3]], k)}")
        assert ex <= bound and ey <= bound, f"{name}: |radii - ref| {ex} / {ey} over the bound {bound}"
        _assert_counts(got, ref, name)


def test_a_bank_against_itself():
    from wu import kid, prdc
    x, _, ref, _ = _real(R.REAL_CASES[1])
    bank = kid.FeatureBank()
    bank.append(torch.from_numpy(x).to(DEV))
    m = prdc.precision_recall_density_coverage(bank, bank, k=3)
    assert m.precision == 1.0 and m.recall == 1.0 and m.coverage == 1.0
    assert isinstance(m, prdc.PRDC) and all(isinstance(v, float) for v in m)
    # the self tiles and the cross tiles run the same operations, so every ball holds its own row and its k nearest: sum(A) >= (k + 1) n
    assert m.density >= 4.0 / 3


def test_two_runs_give_identical_bytes():
    x, y, _, _ = _real(R.REAL_CASES[0])
    a, b = _abi(x, y, 3, 0), _abi(x, y, 3, 0)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    c = _abi(x, y, 3, 3)                           # the radii and the counts do not depend on the split either
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, c))


def test_wrapper_raises_value_errors():
    from wu import prdc
    x = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError, match="k \\+ 1 = 7"):
        prdc.knn_radii(x, 6)
    with pytest.raises(ValueError, match="fake bank has n = 3"):
        prdc.manifold_counts(x, x[:3], 3)
    with pytest.raises(ValueError, match="real bank has n = 2"):
        prdc.precision_recall_density_coverage(x[:2], x, k=5)
    for k in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            prdc.manifold_counts(x, x, k)
    with pytest.raises(ValueError, match="widths 8 / 7"):
        prdc.manifold_counts(x, x[:, :7], 3)
    with pytest.raises(ValueError, match="CUDA"):
        prdc.manifold_counts(x, x.cpu(), 3)
    with pytest.raises(ValueError, match="unit column stride"):
        prdc.knn_radii(x.t(), 3)
    with pytest.raises(ValueError, match="unit column stride"):
        prdc.knn_radii(x.double(), 3)
    assert prdc.knn_radii(x, 5).cpu().tolist() == [0.0] * 6        # n = k + 1, all rows equal


def test_cli_prints_prdc_after_fid_from_feature_npz(tmp_path, capsys):
    """`python -m wu.fid A.npz B.npz --prdc [--kid]`: .npz files holding `features` need no network; without --prdc the output is what it
    was."""
    from wu import fid, prdc
    D, k = 8, 3
    rng = np.random.RandomState(12)
    x = rng.rand(40, D).astype(np.float32)
    y = np.abs(x[rng.randint(0, 40, 33)] + np.exp(rng.uniform(np.log(0.02), np.log(0.8), 33))[:, None] * rng.randn(33, D)).astype(np.float32)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    for path, rows in ((pa, x), (pb, y)):          # mu / sigma too: the run without --prdc / --kid reads nothing else
        np.savez(path, features=rows, mu=rows.astype(np.float64).mean(axis=0), sigma=np.cov(rows.astype(np.float64), rowvar=False))
    ref = R.real(x, y, k)
    assert R.smallest_margin(ref) > R.bound(x, y, D)               # no comparison within rounding of its radius: the counts are decided
    want = R.metrics(ref.A, ref.B, ref.C, k)
    assert 0 < want.precision < 1 and 0 < want.coverage < 1
    base = [pa, pb, "--weights", "unused.pth"]
    kid_args = ["--kid", "--kid-subsets", "4", "--kid-subset-size", "20", "--kid-seed", "3"]

    def run(extra):
        assert fid.main(base + extra) == 0
        return capsys.readouterr().out.strip().splitlines()

    plain, with_kid = run([]), run(kid_args)
    assert len(plain) == 1 and plain[0].startswith("FID: ")
    assert len(with_kid) == 2 and with_kid[0] == plain[0] and with_kid[1].startswith("KID: ") and " ± " in with_kid[1]
    lines = run(["--prdc", "--prdc-k", str(k)])
    assert len(lines) == 2 and lines[0] == plain[0]
    words = lines[1].split()
    assert words[0] == "PRDC:" and words[1::2] == ["precision", "recall", "density", "coverage"] and len(words) == 9
    got = prdc.PRDC(*(float(w) for w in words[2::2]))
    assert got == want
    assert got == fid.calculate_prdc_given_paths([pa, pb], None, k=k)
    both = run(kid_args + ["--prdc", "--prdc-k", str(k)])
    assert both == with_kid + [lines[1]]
    default_k = run(["--prdc"])
    assert R.smallest_margin(R.real(x, y, 5)) > R.bound(x, y, D)
    assert default_k[1] == "PRDC: precision {} recall {} density {} coverage {}".format(*R.prdc(x, y, 5))
    np.savez(str(tmp_path / "c.npz"), mu=np.zeros(D), sigma=np.eye(D))
    with pytest.raises(ValueError, match="features"):
        fid.calculate_prdc_given_paths([pa, str(tmp_path / "c.npz")], None)
