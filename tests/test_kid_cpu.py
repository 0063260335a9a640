"""CPU: Kernel Inception Distance without a GPU -- the numpy restatement (tests/_kid_ref.py) against a literal double loop, the subset draw
of wu.kid.subset_indices, the ValueError cases, the exact integer oracle against the restatement on the grid the GPU test uses, and the
argument errors of the C ABI (wu_kid_workspace_bytes / wu_kid_mmd).  No compute is launched here."""
import numpy as np
import pytest

import _kid_ref as R


def test_restatement_agrees_with_a_literal_double_loop():
    n1, n2, m, D, S = 7, 9, 5, 3, 4
    rng = np.random.RandomState(0)
    X, Y = rng.rand(n1, D).astype(np.float32), rng.rand(n2, D).astype(np.float32)
    degree, gamma, coef0, seed = 3, 1.0 / D, 1.0, 11

    def k(a, b):
        return (gamma * sum(float(a[d]) * float(b[d]) for d in range(D)) + coef0) ** degree

    loop_rng = np.random.RandomState(seed)
    vals = []
    for _ in range(S):
        x = X[loop_rng.choice(n1, m, replace=False)]
        y = Y[loop_rng.choice(n2, m, replace=False)]
        sxx = sum(k(x[i], x[j]) for i in range(m) for j in range(m) if i != j)
        syy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j)
        sxy = sum(k(x[i], y[j]) for i in range(m) for j in range(m))
        vals.append((sxx + syy) / (m * (m - 1)) - 2 * sxy / (m * m))
    mean, std = R.kid(X, Y, num_subsets=S, subset_size=m, degree=degree, gamma=gamma, coef0=coef0, seed=seed)
    # a dozen roundings of O(1) values apart: 1e-13 is a thousand units in the last place of the sums' mean
    assert abs(mean - np.mean(vals)) <= 1e-13 and abs(std - np.std(vals)) <= 1e-13
    sums, mmd2 = R.subsets(X, Y, R.indices(n1, n2, S, m, seed), degree, gamma, coef0)
    np.testing.assert_allclose(mmd2, vals, rtol=0, atol=1e-13)
    assert sums.shape == (S, 3)


def test_subset_indices_reproduce_the_draw_order():
    from wu import kid
    n1, n2, S, m, seed = 11, 8, 6, 5, 2020
    idx = kid.subset_indices(n1, n2, S, m, seed)
    assert idx.shape == (S, 2, m) and idx.dtype == np.int32
    rng = np.random.RandomState(seed)
    for s in range(S):
        np.testing.assert_array_equal(idx[s, 0], rng.choice(n1, m, replace=False))      # the first bank's rows first,
        np.testing.assert_array_equal(idx[s, 1], rng.choice(n2, m, replace=False))      # then the second's
        assert len(set(idx[s, 0])) == m and len(set(idx[s, 1])) == m
    assert idx[:, 0].max() < n1 and idx[:, 1].max() < n2 and idx.min() >= 0
    np.testing.assert_array_equal(idx, kid.subset_indices(n1, n2, S, m, seed))         # seed-stable
    np.testing.assert_array_equal(idx, R.indices(n1, n2, S, m, seed))
    assert not np.array_equal(idx, kid.subset_indices(n1, n2, S, m, seed + 1))


@pytest.mark.parametrize("n1,n2,m", [(500, 700, 1000), (700, 500, 501), (10, 10, 1), (10, 10, 0)])
def test_subset_size_errors(n1, n2, m):
    from wu import kid
    with pytest.raises(ValueError) as e:
        kid.subset_indices(n1, n2, 3, m, 0)
    msg = str(e.value)
    assert str(n1) in msg and str(n2) in msg and str(m) in msg and "subset_size" in msg and "lower" in msg


def test_kernel_inception_distance_refuses_host_rows_and_oversized_subsets():
    import torch
    from wu import features, kid
    assert kid.FeatureBank is features.FeatureBank                 # one class under its documented name and its new home
    with pytest.raises(ValueError, match="CUDA"):
        kid.kernel_inception_distance(torch.zeros(4, 3), torch.zeros(4, 3), subset_size=2)        # no host fallback
    with pytest.raises(ValueError, match="CUDA"):
        kid.FeatureBank().append(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="no rows"):
        kid.FeatureBank().features


@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_integer_oracle_equals_the_restatement_bit_for_bit(case):
    n1, n2, m, D, S, degree, coef0 = case
    x, y, idx = R.exact_case(case)
    assert idx.shape == (S, 2, m) and n1 - 1 in idx[0, 0] and n2 - 1 in idx[0, 1]
    assert all(len(set(r)) == m for sub in idx for r in sub)
    exact = R.exact_sums(x, y, idx, degree, R.GAMMA_DEN, coef0)
    sums, _ = R.subsets(x, y, idx, degree, 1.0 / R.GAMMA_DEN, float(coef0))
    assert np.array_equal(exact, sums), f"restatement differs from the integer oracle: {np.abs(exact - sums).max()}"


def test_workspace_and_argument_errors_are_reported_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_kid_workspace_bytes(1, 2) == 3 * 8                        # one tile per block
    assert lib.wu_kid_workspace_bytes(5, 64) == 5 * 3 * 8
    assert lib.wu_kid_workspace_bytes(5, 65) == 5 * (3 + 3 + 4) * 8        # T = 2: 3 + 3 upper-triangular tiles and 4 of xy
    assert lib.wu_kid_workspace_bytes(100, 1000) == 100 * (136 + 136 + 256) * 8
    assert lib.wu_kid_workspace_bytes(1, 1) == 0 and lib.wu_kid_workspace_bytes(0, 64) == 0 and lib.wu_kid_workspace_bytes(65536, 64) == 0
    p = 64       # any non-NULL address: every call below is refused before a launch

    def call(x=p, ldx=8, n1=10, y=p, ldy=8, n2=12, idx=p, S=3, m=5, D=8, degree=3, ws=p, sums=p, mmd2=p):
        return lib.wu_kid_mmd(x, ldx, n1, y, ldy, n2, idx, S, m, D, degree, 0.125, 1.0, ws, sums, mmd2, None)

    for kwargs, word in ((dict(m=1), b"at least 2"), (dict(m=11), b"min(n1 10, n2 12)"), (dict(n2=4), b"min(n1 10, n2 4)"),
                         (dict(degree=0), b"degree"), (dict(S=65536), b"65535"), (dict(S=0), b"65535"), (dict(ldx=7), b"ldx 7"),
                         (dict(ldy=7), b"ldy 7"), (dict(x=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(ws=None), b"NULL"),
                         (dict(mmd2=None), b"NULL")):
        assert call(**kwargs) < 0, kwargs
        assert word in lib.wu_last_error(), (kwargs, lib.wu_last_error())
