"""Kernel Inception Distance restated in numpy float64 (what wu.kid computes, tests/test_kid_cpu.py and tests/test_gpu_kid.py), and an exact
integer oracle for small-integer features.

Semantics: rng = np.random.RandomState(seed); per subset i1 = rng.choice(n1, m, replace=False), then i2 = rng.choice(n2, m, replace=False);
k(x, y) = (gamma <x, y> + coef0)^degree in float64 on the float32 rows widened to float64, the power by repeated multiplication;
sxx = sum_{i != j} k(x_i, x_j), syy likewise, sxy = sum_{i, j} k(x_i, y_j); mmd2 = (sxx + syy) / (m (m - 1)) - 2 sxy / (m m);
the result is (np.mean, np.std) of the subsets' mmd2."""
import numpy as np

U = 2.0 ** -53      # unit roundoff of float64


def indices(n1, n2, num_subsets, subset_size, seed):
    if subset_size < 2 or subset_size > min(n1, n2):
        raise ValueError(f"subset_size {subset_size} outside 2..min({n1}, {n2})")
    rng = np.random.RandomState(seed)
    out = np.empty((num_subsets, 2, subset_size), dtype=np.int32)
    for s in range(num_subsets):
        out[s, 0] = rng.choice(n1, subset_size, replace=False)
        out[s, 1] = rng.choice(n2, subset_size, replace=False)
    return out


def poly_kernel(a, b, degree, gamma, coef0):
    t = gamma * (a.astype(np.float64) @ b.astype(np.float64).T) + coef0
    k = t.copy()
    for _ in range(degree - 1):
        k = k * t
    return k


def mmd2_of(sxx, syy, sxy, m):
    return (sxx + syy) / (m * (m - 1)) - 2 * sxy / (m * m)


def subset_sums(x, y, degree, gamma, coef0):
    """(sxx, syy, sxy) of one subset: x, y (m, D)."""
    kxx, kyy, kxy = (poly_kernel(a, b, degree, gamma, coef0) for a, b in ((x, x), (y, y), (x, y)))
    np.fill_diagonal(kxx, 0.0)
    np.fill_diagonal(kyy, 0.0)
    return float(kxx.sum()), float(kyy.sum()), float(kxy.sum())


def subsets(X, Y, idx, degree=3, gamma=None, coef0=1.0):
    """sums (S, 3) and mmd2 (S,) of the subsets idx (S, 2, m) of X (n1, D) and Y (n2, D)."""
    X, Y = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    if gamma is None:
        gamma = 1.0 / X.shape[1]
    m = idx.shape[2]
    sums = np.array([subset_sums(X[i[0]], Y[i[1]], degree, gamma, coef0) for i in idx], dtype=np.float64).reshape(-1, 3)
    mmd2 = np.array([mmd2_of(s[0], s[1], s[2], m) for s in sums], dtype=np.float64)
    return sums, mmd2


def kid(X, Y, num_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=2020):
    idx = indices(len(X), len(Y), num_subsets, subset_size, seed)
    _, mmd2 = subsets(X, Y, idx, degree, gamma, coef0)
    return float(np.mean(mmd2)), float(np.std(mmd2))


def bound(sums, m, D):
    """Per subset: 32 (D + 2) 2^-53 kbar, kbar the largest of the three block means of k.  Derived, not measured: the worst-case rounding
    bound for two float64 dot-product-then-cube evaluations of non-negative terms, times the weights 1 + 1 + 2 of the mmd2 combination."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    kbar = np.maximum(np.maximum(sums[:, 0], sums[:, 1]) / (m * (m - 1)), sums[:, 2] / (m * m))
    return 32 * (D + 2) * U * kbar


def exact_sums(xi, yi, idx, degree, gamma_den, coef0):
    """The integer oracle.  xi, yi: integer feature rows; gamma = 1 / gamma_den with gamma_den a power of two; coef0 a non-negative integer.
    Then k = (g + coef0 gamma_den)^degree / gamma_den^degree with g an integer: the sums are Python integers over a power of two, and as
    long as they stay below 2^53 the float64 value is exact whatever the order of summation.  Returns sums (S, 3) float64."""
    assert gamma_den & (gamma_den - 1) == 0 and int(coef0) == coef0 and coef0 >= 0
    xi, yi = np.asarray(xi).astype(np.int64), np.asarray(yi).astype(np.int64)
    scale = gamma_den ** degree
    out = np.empty((len(idx), 3), dtype=np.float64)
    for s, i in enumerate(idx):
        x, y = xi[i[0]], yi[i[1]]
        tot = []
        for a, b, offdiag in ((x, x, True), (y, y, True), (x, y, False)):
            t = (a @ b.T + int(coef0) * gamma_den).astype(object)        # Python integers: no overflow
            k = t ** degree
            if offdiag:
                np.fill_diagonal(k, 0)
            tot.append(int(k.sum()))
        assert max(tot) < 2 ** 53
        out[s] = [v / scale for v in tot]        # exact: an integer below 2^53 over a power of two
    return out


# ---- the exact grid of tests/test_gpu_kid.py (and of the bit-for-bit CPU check): (n1, n2, m, D, S, degree, coef0) -------------------------
# features in {0, 1, 2, 3}, gamma = 1 / 64: every product, power and partial sum is a multiple of 2^-18 below 2^53
GAMMA_DEN = 64
EXACT_GRID = [(m + 6, m + 1, m, D, S, 3, 1)
              for m in (2, 63, 64, 65, 129)        # smallest legal; the tile edge; three tiles per side (diagonal, weighted, ragged)
              for D in (1, 7, 64, 100)             # 100: K-chunk tail
              for S in (1, 5)]
EXACT_GRID += [(131, 150, 129, 7, 1, 1, 1),        # degree 1
               (70, 66, 65, 64, 5, 2, 1),          # degree 2
               (66, 70, 65, 7, 1, 3, 0)]           # coef0 = 0


def exact_case_id(c):
    return "n%dx%d_m%d_D%d_S%d_deg%d_c%d" % c


def exact_case(c):
    """Integer features in {0..3} (as float32) and subset indices; the last row of each bank is always drawn (an index equal to n - 1)."""
    n1, n2, m, D, S, degree, coef0 = c
    rng = np.random.RandomState(1000 * m + 10 * D + S)
    x = rng.randint(0, 4, (n1, D)).astype(np.float32)
    y = rng.randint(0, 4, (n2, D)).astype(np.float32)
    idx = indices(n1, n2, S, m, seed=m + D)
    for side, n, pos in ((0, n1, m - 1), (1, n2, 0)):
        if n - 1 not in idx[0, side]:
            idx[0, side, pos] = n - 1
    return x, y, idx
