"""Top-k nearest-neighbour retrieval restated in numpy on tests/_prdc_ref.dist2 (what wu.retrieval.topk computes; tests/test_nn_cpu.py and
tests/test_gpu_nn.py): an exact int64 path for integer features and an np.longdouble path for real ones.

Semantics.  d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0) as in _prdc_ref.  Row i of the result holds the k smallest pairs (d2(q_i, b_c), c)
over the bank columns c in the lexicographic order -- smaller d2 first, on equal d2 the smaller c -- which is np.lexsort((c, d2)).  With
``self_offset`` s >= 0, query row i is bank row s + i and that one column is left out."""
import numpy as np

import _prdc_ref as P

MAX_K = 16


def sorted_rows(d, m, self_offset=-1):
    """Per row of the (nq, nb) matrix ``d`` its m smallest (d2, column) pairs in the lexicographic order, column self_offset + i left out
    of row i: (d2 (nq, m), columns (nq, m) int64).  No check on m."""
    nq, nb = d.shape
    cols = np.arange(nb)
    dist2 = np.empty((nq, m), dtype=d.dtype)
    index = np.empty((nq, m), dtype=np.int64)
    for i in range(nq):
        keep = cols != self_offset + i if self_offset >= 0 else np.ones(nb, dtype=bool)
        c, v = cols[keep], d[i, keep]
        order = np.lexsort((c, v))[:m]
        index[i], dist2[i] = c[order], v[order]
    return dist2, index


def topk_of(d, k, self_offset=-1):
    """(dist2 (nq, k), index (nq, k) int64) from the (nq, nb) matrix ``d``, with the library's argument checks."""
    nq, nb = d.shape
    if k < 1 or k > MAX_K:
        raise ValueError(f"k {k} outside 1..{MAX_K}")
    if nb < k + (1 if self_offset >= 0 else 0):
        raise ValueError(f"nb {nb} bank rows, k {k} needs {'k + 1' if self_offset >= 0 else 'k'}")
    if self_offset >= 0 and self_offset + nq > nb:
        raise ValueError(f"self_offset {self_offset} + nq {nq} over nb {nb}")
    return sorted_rows(d, k, self_offset)


def exact(q, b, k, self_offset=-1):
    """The integer oracle: every d2 is an int64, exact whatever the order of summation."""
    return topk_of(P.dist2(np.asarray(q).astype(np.int64), np.asarray(b).astype(np.int64), np.int64), k, self_offset)


def real(q, b, k, self_offset=-1):
    """The np.longdouble restatement on float32 rows."""
    return topk_of(P.dist2(np.asarray(q, dtype=np.float32), np.asarray(b, dtype=np.float32), np.longdouble), k, self_offset)


def smallest_gap(q, b, k, self_offset=-1):
    """The smallest difference between consecutive entries of any row's top k + 1 (the bank must hold that many columns): while it
    exceeds twice the bound on one d2, rounding can change neither which columns are the k nearest nor their order."""
    d = P.dist2(np.asarray(q, dtype=np.float32), np.asarray(b, dtype=np.float32), np.longdouble)
    top, _ = sorted_rows(d, k + 1, self_offset)
    return float(np.diff(top, axis=1).min())


def ties_inside(q, b, m, self_offset=-1):
    """Number of rows of the integer case with two equal d2 among their m nearest: the index rule orders them."""
    top, _ = sorted_rows(P.dist2(np.asarray(q).astype(np.int64), np.asarray(b).astype(np.int64), np.int64), m, self_offset)
    return int((np.diff(top, axis=1) == 0).any(axis=1).sum())


def ties_across(q, b, k, self_offset=-1):
    """Number of rows of the integer case whose k-th and (k + 1)-th nearest lie at the same d2: only the index rule decides which of
    the two is kept."""
    top, _ = sorted_rows(P.dist2(np.asarray(q).astype(np.int64), np.asarray(b).astype(np.int64), np.int64), k + 1, self_offset)
    return int((top[:, k] == top[:, k - 1]).sum())


# ---- the exact grid: (nq, nb, D, k, exclude_self); features in {0..3} -----------------------------------------------------------------------
EXACT_GRID = [(1, 1, 1, 1, False),          # nb == k, the smallest shape
              (2, 16, 4, 16, False),        # nb == k at the largest k
              (65, 64, 33, 3, False),       # tile edge and K-chunk tail
              (64, 65, 32, 1, False),
              (70, 130, 70, 5, False),      # three column tiles
              (17, 150, 33, 16, False),     # ties across the k = 16 boundary
              (129, 129, 31, 5, True)]      # a bank against itself
COL_SPLITS = (0, 1, 2, 3)


def exact_case_id(c):
    return "nq%d_nb%d_D%d_k%d%s" % (c[0], c[1], c[2], c[3], "_self" if c[4] else "")


def exact_case(c):
    """(query, bank) float32 with integer features in {0..3}, drawn by _prdc_ref.exact_case.  A shape of its grid is taken as it stands
    there: (17, 150, 33, 16) is its x / y, (70, 130, 70, 5) the y / x of its (130, 70, 70, 5).  The self case queries x against itself."""
    nq, nb, D, k, self_ = c
    if self_:
        x, _ = P.exact_case((nb, nb, D, k))
        return x, x
    if (nq, nb, D, k) not in P.EXACT_GRID and (nb, nq, D, k) in P.EXACT_GRID:
        bank, query = P.exact_case((nb, nq, D, k))
        return query, bank
    return P.exact_case((nq, nb, D, k))


def three_copies_case():
    """(query, bank, k): bank rows 0, 64 and 128 identical and equal to query row 2 -- a tie at d2 = 0 across three column tiles (and, with
    2 or 3 splits, across splits), which only the index rule resolves.  k = 2 keeps rows 0 and 64 and must drop row 128."""
    rng = np.random.RandomState(77)
    bank = rng.randint(0, 4, (130, 9)).astype(np.float32)
    query = rng.randint(0, 4, (5, 9)).astype(np.float32)
    bank[64] = bank[0]
    bank[128] = bank[0]
    query[2] = bank[0]
    return query, bank, 2


# ---- real features: _prdc_ref.real_case (n1, n2, k-of-its-own) with the k used here; D = 2048 ---------------------------------------------------
REAL_CASES = [((140, 129, 3), 8), ((70, 133, 5), 16)]
