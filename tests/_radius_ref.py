"""The radius join and the per-row ball scores restated in numpy on tests/_prdc_ref.dist2 (what wu.retrieval.radius_join and
wu.retrieval.ball_scores compute; tests/test_radius_cpu.py and tests/test_gpu_radius.py): an exact int64 path for integer features and an
np.longdouble path for real ones.

Semantics.  d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0) as in _prdc_ref.  With ``self_offset`` s >= 0, query row i is bank row s + i.
Join: the pair (i, c) is a member when d2(q_i, b_c) <= radius2, c != s + i with s >= 0, and c > s + i with ``upper_only``; the result is CSR,
rows ascending and columns ascending within a row.
Ball scores, with the bank's squared radii r2 and over the columns j != s + i:  count[i] = #{j : d2_ij <= r2_j};  rarity_r2[i] the smallest
r2_j among those (+inf without one), rarity_index[i] its column, the smaller on equal radii (-1 without one);  the realism pair is the
maximiser of rho_ij = r2_j / d2_ij (+inf when d2_ij == 0, whatever r2_j), the smaller j on equal rho."""
import collections

import numpy as np

import _nn_ref as N
import _prdc_ref as P

MAX_N = 1 << 21

Ball = collections.namedtuple("Ball", ["count", "rarity_r2", "rarity_index", "realism_r2", "realism_d2", "realism_index", "rho"])


def _check(nq, nb, self_offset):
    if not (1 <= nq <= MAX_N and 1 <= nb <= MAX_N):
        raise ValueError(f"nq {nq} / nb {nb} outside 1..{MAX_N}")
    if self_offset < -1:
        raise ValueError(f"self_offset {self_offset} (-1: none)")
    if self_offset >= 0 and self_offset + nq > nb:
        raise ValueError(f"self_offset {self_offset} + nq {nq} over nb {nb}")


def allowed(nq, nb, self_offset=-1, upper_only=False):
    """(nq, nb) bool: the columns a row may pair with."""
    own = self_offset + np.arange(nq)[:, None]
    cols = np.arange(nb)[None, :]
    if upper_only:
        return cols > own
    return cols != own if self_offset >= 0 else np.ones((nq, nb), dtype=bool)


def join_of(d, radius2, self_offset=-1, upper_only=False):
    """(row_ptr (nq + 1) int64, index int64, dist2 in d's dtype) from the (nq, nb) matrix ``d``, with the library's argument checks."""
    nq, nb = d.shape
    _check(nq, nb, self_offset)
    if not (np.isfinite(radius2) and radius2 >= 0):
        raise ValueError(f"radius2 {radius2} must be finite and >= 0")
    if upper_only and self_offset < 0:
        raise ValueError("upper_only needs a self_offset >= 0")
    m = (d <= radius2) & allowed(nq, nb, self_offset, upper_only)
    rows, cols = np.nonzero(m)                     # row-major: rows ascending, columns ascending within a row
    row_ptr = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)
    return row_ptr, cols.astype(np.int64), d[rows, cols]


def exact_d(q, b):
    return P.dist2(np.asarray(q).astype(np.int64), np.asarray(b).astype(np.int64), np.int64)


def real_d(q, b):
    return P.dist2(np.asarray(q, dtype=np.float32), np.asarray(b, dtype=np.float32), np.longdouble)


def exact(q, b, radius2, self_offset=-1, upper_only=False):
    """The integer oracle: every d2 is an int64, exact whatever the order of summation."""
    return join_of(exact_d(q, b), radius2, self_offset, upper_only)


def real(q, b, radius2, self_offset=-1, upper_only=False):
    """The np.longdouble restatement on float32 rows."""
    return join_of(real_d(q, b), radius2, self_offset, upper_only)


def ball_of(d, r2, self_offset=-1, ftype=np.float64):
    """The Ball of the (nq, nb) matrix ``d`` and the nb squared radii ``r2``; quotients in ``ftype`` (one division per pair: for exact
    integers in float64 numpy's correctly rounded quotient)."""
    nq, nb = d.shape
    _check(nq, nb, self_offset)
    if self_offset >= 0 and nb < 2:
        raise ValueError(f"nb {nb} bank rows, need at least 2 with the row itself excluded")
    ok = allowed(nq, nb, self_offset)
    r = np.broadcast_to(np.asarray(r2)[None, :], d.shape)
    inside = (d <= r) & ok
    count = inside.sum(axis=1).astype(np.int64)
    masked = np.where(inside, r.astype(ftype), np.inf)
    rarity_index = np.where(count > 0, masked.argmin(axis=1), -1).astype(np.int64)     # argmin: the first of equal radii
    rarity_r2 = masked.min(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(d == 0, np.inf, r.astype(ftype) / d.astype(ftype))
    rho = np.where(ok, rho, -np.inf)
    j = rho.argmax(axis=1).astype(np.int64)        # argmax: the first of equal quotients
    i = np.arange(nq)
    return Ball(count, rarity_r2, rarity_index, r[i, j], d[i, j], j, rho[i, j])


def exact_ball(q, b, k, self_offset=-1):
    """(Ball, r2): the integer oracle with the bank's exact squared k-NN radii."""
    r2 = P.radii_of(exact_d(b, b), k)
    return ball_of(exact_d(q, b), r2, self_offset), r2


def real_ball(q, b, k, self_offset=-1):
    r2 = P.radii_of(real_d(b, b), k)
    return ball_of(real_d(q, b), r2, self_offset, np.longdouble), r2


# ---- the exact grid: _nn_ref's shapes (its k is not used here) with four radii each -----------------------------------------------------------
EXACT_GRID = N.EXACT_GRID
COL_SPLITS = N.COL_SPLITS
BALL_KS = (1, 3)
exact_case_id = N.exact_case_id
exact_case = N.exact_case


def self_offset_of(case):
    return 0 if case[4] else -1


def off_self(d, self_offset=-1):
    """The sorted d2 of the pairs a row may form."""
    return np.sort(d[allowed(d.shape[0], d.shape[1], self_offset)])


def exact_radii(case):
    """0, the entries at len // 20 and len // 2 of the sorted off-self d2, and the maximum."""
    q, b = exact_case(case)
    v = off_self(exact_d(q, b), self_offset_of(case))
    return [0, int(v[len(v) // 20]), int(v[len(v) // 2]), int(v[-1])]


# ---- real features: _prdc_ref.real_case; (case, query side, self_offset, the 2 % and 25 % quantiles of the off-self d2 as literals) -----------
REAL_JOINS = [((140, 129, 3), "y", -1, (332.0, 354.5)),
              ((140, 129, 3), "x", 0, (323.5, 335.75)),
              ((70, 133, 5), "y", -1, (326.0, 351.0)),
              ((70, 133, 5), "x", 0, (323.0, 334.75))]
REAL_BALL_KS = {(140, 129, 3): 3, (70, 133, 5): 5}


def real_rows(pc, side):
    """(query, bank) of a real case: the fakes y against the reals x, or x against itself."""
    x, y = P.real_case(pc)
    return (y, x) if side == "y" else (x, x)


def join_margin(d, radius2, self_offset=-1):
    """min |d2 - radius2| over the pairs a row may form: while it exceeds twice the bound on one d2, rounding cannot change the members."""
    return float(np.abs(off_self(d, self_offset) - radius2).min())


def ball_margins(d, r2, self_offset=-1):
    """(membership, realism, rarity): min |d2_ij - r2_j| over the allowed pairs; the smallest relative gap between any row's largest and
    second largest quotient; the smallest gap between the two smallest radii among any row's balls (inf where no row has two).  While
    they exceed the error of their quantities, rounding changes neither count nor either index."""
    nq, nb = d.shape
    ok = allowed(nq, nb, self_offset)
    r = np.broadcast_to(np.asarray(r2)[None, :], d.shape)
    member = float(np.abs(d - r)[ok].min())
    rho = np.where(ok, r / np.maximum(d, np.finfo(np.float64).tiny), -np.inf)
    top = -np.sort(-rho, axis=1)[:, :2]
    realism = float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) if nb - (self_offset >= 0) >= 2 else np.inf
    inside = np.sort(np.where((d <= r) & ok, r, np.inf), axis=1)[:, :2] if nb >= 2 else np.full((nq, 2), np.inf)
    two = np.isfinite(inside[:, 1])
    rarity = float((inside[two, 1] - inside[two, 0]).min()) if two.any() else np.inf
    return member, realism, rarity
