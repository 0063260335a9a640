"""Improved precision / recall and density / coverage restated in numpy (what wu.prdc computes; tests/test_prdc_cpu.py and
tests/test_gpu_prdc.py): an exact int64 path for integer features and an np.longdouble path for real ones.

Semantics (the prdc package's, on squared distances).  For float32 rows a, b widened to float64,
d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0).  radius_X[i] is the (k + 1)-th smallest of row i of the n x n matrix d2(x_i, x_j) with the
diagonal forced to 0: the row itself is one of the k + 1.  With X real (n1 rows), Y fake (n2 rows) and `<=`:
    A[i] = #{j : d2(x_i, y_j) <= radius_X[i]}    B[i] = #{j : d2(x_i, y_j) <= radius_Y[j]}    C[j] = #{i : d2(x_i, y_j) <= radius_X[i]}
    precision = mean(C > 0)   recall = mean(B > 0)   density = sum(C) / (k n2)   coverage = mean(A > 0)"""
import collections

import numpy as np

U = 2.0 ** -53      # unit roundoff of float64
MAX_K = 16

PRDC = collections.namedtuple("PRDC", ["precision", "recall", "density", "coverage"])
Result = collections.namedtuple("Result", ["radii_x", "radii_y", "A", "B", "C", "dxy"])


def dist2(a, b, dtype):
    """(len(a), len(b)) squared distances in `dtype` (np.int64: exact for integer features; np.longdouble for real ones)."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    na, nb = (a * a).sum(axis=1), (b * b).sum(axis=1)
    g = a @ b.T
    return np.maximum((na[:, None] + nb[None, :]) - 2 * g, 0)


def radii_of(dself, k):
    """The (k + 1)-th smallest of every row of the square matrix `dself`, its diagonal forced to 0."""
    n = dself.shape[0]
    if k < 1 or k > MAX_K:
        raise ValueError(f"k {k} outside 1..{MAX_K}")
    if n < k + 1:
        raise ValueError(f"n {n} rows, k {k} needs k + 1")
    d = dself.copy()
    np.fill_diagonal(d, 0)
    return np.sort(d, axis=1)[:, k]


def counts_of(dxy, rx, ry):
    in_x = dxy <= rx[:, None]
    in_y = dxy <= ry[None, :]
    return in_x.sum(axis=1).astype(np.int64), in_y.sum(axis=1).astype(np.int64), in_x.sum(axis=0).astype(np.int64)


def compute(x, y, k, dtype):
    rx, ry = radii_of(dist2(x, x, dtype), k), radii_of(dist2(y, y, dtype), k)
    dxy = dist2(x, y, dtype)
    A, B, C = counts_of(dxy, rx, ry)
    return Result(rx, ry, A, B, C, dxy)


def exact(xi, yi, k):
    """The integer oracle: every d2 is an int64, exact whatever the order of summation."""
    return compute(np.asarray(xi).astype(np.int64), np.asarray(yi).astype(np.int64), k, np.int64)


def real(x, y, k):
    """The np.longdouble restatement on float32 rows."""
    return compute(np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32), k, np.longdouble)


def metrics(A, B, C, k):
    n1, n2 = len(A), len(C)
    return PRDC(int((C > 0).sum()) / n2, int((B > 0).sum()) / n1, int(C.sum()) / (k * n2), int((A > 0).sum()) / n1)


def prdc(x, y, k=5):
    """The four metrics of float32 rows through the longdouble path."""
    r = real(x, y, k)
    return metrics(r.A, r.B, r.C, k)


def bound(x, y, D):
    """4 (D + 2) 2^-53 (max_i |x_i|^2 + max_j |y_j|^2), on one d2.  Derived, not measured: a float64 sum of D non-negative squares carries
    at most D u of itself in any order, so the two norms together D u (|a|^2 + |b|^2); the dot product at most D u sum |a_d b_d|
    <= D u (|a|^2 + |b|^2) / 2, doubled by the factor 2; adding the norms and the subtraction round once each on values of at most
    2 (|a|^2 + |b|^2): (2 D + 3) u (|a|^2 + |b|^2) to first order, and 4 (D + 2) leaves a factor of two for the higher-order terms."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return 4 * (D + 2) * U * float((x * x).sum(axis=1).max() + (y * y).sum(axis=1).max())


def ties(r):
    """Number of pairs with d2 exactly equal to a radius it is compared with: what `<=` against `<` decides."""
    return int((r.dxy == r.radii_x[:, None]).sum() + (r.dxy == r.radii_y[None, :]).sum())


def smallest_margin(r):
    """min |d2 - radius| over every comparison the counts make."""
    return float(min(np.abs(r.dxy - r.radii_x[:, None]).min(), np.abs(r.dxy - r.radii_y[None, :]).min()))


# ---- the exact grid: (n1, n2, D, k); features in {0, 1, 2, 3} -------------------------------------------------------------------------------
EXACT_GRID = [(2, 2, 4, 1),          # smallest legal shape
              (4, 6, 5, 3),          # n1 = k + 1
              (65, 64, 33, 3),       # tile edge and K-chunk tail
              (64, 65, 32, 1),       # duplicate rows: radius 0
              (130, 70, 70, 5),      # three row tiles
              (17, 150, 33, 16),     # largest k
              (129, 129, 31, 5)]     # equal bank sizes, three tiles per side
COL_SPLITS = (0, 1, 2, 3)


def exact_case_id(c):
    return "n%dx%d_D%d_k%d" % c


def exact_case(c):
    """Integer features in {0..3} as float32.  With n1 > 8, x[3] = x[1] and y[5] = x[1]: duplicate rows within a bank and across the banks."""
    n1, n2, D, k = c
    rng = np.random.RandomState(1000 * n1 + n2)
    x = rng.randint(0, 4, (n1, D)).astype(np.float32)
    y = rng.randint(0, 4, (n2, D)).astype(np.float32)
    if n1 > 8:
        x[3] = x[1]
        y[5] = x[1]
    return x, y


# ---- real features: (n1, n2, k), D = 2048 ----------------------------------------------------------------------------------------------------
REAL_D = 2048
REAL_CASES = [(140, 129, 3), (70, 133, 5)]


def real_case(c):
    """x = rand(n1, D); y_j = |x[src_j] + sigma_j randn(D)| with sigma_j log-uniform in [0.05, 0.6]: fakes from close to a real row to far
    from every one, so that A and C hold zeros and non-zeros."""
    n1, n2, k = c
    rng = np.random.RandomState(n1)
    x = rng.rand(n1, REAL_D).astype(np.float32)
    src = rng.randint(0, n1, n2)
    sigma = np.exp(rng.uniform(np.log(0.05), np.log(0.6), n2))
    y = np.abs(x[src] + sigma[:, None] * rng.randn(n2, REAL_D)).astype(np.float32)
    return x, y
