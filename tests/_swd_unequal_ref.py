"""The W1 distance of two sorted samples of unequal length, twice: the closed form of wu/swd.py's "Distance" paragraph in numpy (int64
weights, float64 terms, vectorised), which the kernel must reproduce, and ``exact``: rational arithmetic over the merged breakpoints of the
two quantile functions, which knows nothing of the closed form.  The oracle of tests/test_swd_unequal_cpu.py and
tests/test_gpu_swd_unequal.py; it imports nothing from the package."""
import fractions

import numpy as np


def weights(ml, ms):
    """(j0, j1, w0, w1), int64 arrays over i < ml, for a longer column of ml keys against a shorter one of ms <= ml: in units of
    1 / (ml ms), x_i owns [i ms, (i + 1) ms) and y_j owns [j ml, (j + 1) ml); x_i meets y_j0 over w0 units and y_j1 over w1."""
    ml, ms = int(ml), int(ms)
    assert 1 <= ms <= ml
    i = np.arange(ml, dtype=np.int64)
    lo = i * ms
    hi = lo + ms
    j0 = lo // ml
    j1 = (hi - 1) // ml
    mid = np.minimum(hi, (j0 + 1) * ml)
    return j0, j1, mid - lo, hi - mid


def closed_form_rows(a, b):
    """(ndirs,) float64: a (ndirs, m1), b (ndirs, m2), rows ascending.  The walk is over the longer rows (a's when m1 == m2)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    x, y = (a, b) if a.shape[1] >= b.shape[1] else (b, a)
    ml, ms = x.shape[1], y.shape[1]
    j0, j1, w0, w1 = weights(ml, ms)
    terms = np.empty((x.shape[0], ml, 2), dtype=np.float64)
    terms[:, :, 0] = w0.astype(np.float64) * np.abs(x - y[:, j0])
    terms[:, :, 1] = w1.astype(np.float64) * np.abs(x - y[:, j1])
    return terms.reshape(x.shape[0], -1).sum(axis=1) / np.float64(ml * ms)


def closed_form(a, b):
    """The same for two 1-D samples in any order."""
    return float(closed_form_rows(np.sort(np.asarray(a, dtype=np.float64))[None], np.sort(np.asarray(b, dtype=np.float64))[None])[0])


def exact(a, b):
    """fractions.Fraction: the integral of |Fa^-1(t) - Fb^-1(t)| over [0, 1] for two 1-D samples in any order.  With t in units of
    1 / (m1 m2), Fa^-1 is constant between the multiples of m2 and Fb^-1 between those of m1: the integrand is constant between two
    neighbours of the merged breakpoints {i m2} | {j m1}."""
    a, b = sorted(fractions.Fraction(float(v)) for v in a), sorted(fractions.Fraction(float(v)) for v in b)
    m1, m2 = len(a), len(b)
    points = sorted(set(range(0, m1 * m2 + 1, m2)) | set(range(0, m1 * m2 + 1, m1)))
    total = fractions.Fraction(0)
    for p, q in zip(points[:-1], points[1:]):
        total += (q - p) * abs(a[p // m2] - b[p // m1])
    return total / (m1 * m2)
