"""CPU: improved precision / recall and density / coverage without a GPU -- the numpy restatement (tests/_prdc_ref.py) against a literal,
sort-based computation on tiny cases, the properties of the case lists the GPU test relies on (ties on the exact grid, margins on the real
features), the argument errors of the C ABI (wu_prdc_workspace_bytes / wu_knn_radii / wu_prdc_counts) and the validation of wu.prdc on
host tensors.  No compute is launched here."""
import numpy as np
import pytest

import _prdc_ref as R


def _brute(x, y, k):
    """Python floats / integers, one pair at a time; the radius through sorted()."""
    def d2(a, b):
        na, nb, g = sum(v * v for v in a), sum(v * v for v in b), sum(u * v for u, v in zip(a, b))
        return max((na + nb) - 2 * g, 0)

    def radii(rows):
        return [sorted(0 if i == j else d2(rows[i], rows[j]) for j in range(len(rows)))[k] for i in range(len(rows))]

    rx, ry = radii(x), radii(y)
    A = [sum(d2(a, b) <= rx[i] for b in y) for i, a in enumerate(x)]
    B = [sum(d2(a, b) <= ry[j] for j, b in enumerate(y)) for a in x]
    C = [sum(d2(a, b) <= rx[i] for i, a in enumerate(x)) for b in y]
    return rx, ry, A, B, C


@pytest.mark.parametrize("n1,n2,D,k", [(2, 2, 3, 1), (5, 7, 2, 2), (9, 4, 6, 3), (18, 20, 3, 16)])
def test_integer_oracle_agrees_with_a_literal_sort(n1, n2, D, k):
    rng = np.random.RandomState(n1 + n2)
    x, y = rng.randint(0, 4, (n1, D)), rng.randint(0, 4, (n2, D))
    if n1 > 4:
        x[2] = x[0]          # a duplicate row
    rx, ry, A, B, C = _brute([[int(v) for v in r] for r in x], [[int(v) for v in r] for r in y], k)
    r = R.exact(x, y, k)
    assert r.radii_x.tolist() == rx and r.radii_y.tolist() == ry
    assert r.A.tolist() == A and r.B.tolist() == B and r.C.tolist() == C
    assert sum(A) == sum(C)
    # the longdouble path on the same integers gives the same numbers
    q = R.real(x.astype(np.float32), y.astype(np.float32), k)
    assert np.array_equal(q.radii_x, rx) and np.array_equal(q.A, A) and np.array_equal(q.B, B) and np.array_equal(q.C, C)


def test_real_restatement_agrees_with_a_literal_sort():
    n1, n2, D, k = 7, 9, 5, 2
    rng = np.random.RandomState(1)
    x, y = rng.rand(n1, D).astype(np.float32), rng.rand(n2, D).astype(np.float32)
    rx, ry, A, B, C = _brute([[float(v) for v in r] for r in x], [[float(v) for v in r] for r in y], k)
    r = R.real(x, y, k)
    # float64 loops against longdouble matrices: a dozen roundings of O(1) values apart
    np.testing.assert_allclose(r.radii_x.astype(np.float64), rx, rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.radii_y.astype(np.float64), ry, rtol=0, atol=1e-13)
    assert R.smallest_margin(r) > 1e-9          # so no comparison can differ between the two
    assert r.A.tolist() == A and r.B.tolist() == B and r.C.tolist() == C
    m = R.prdc(x, y, k)
    assert m == R.metrics(r.A, r.B, r.C, k) and m.density == sum(C) / (k * n2) and m.precision == sum(c > 0 for c in C) / n2
    assert m.recall == sum(b > 0 for b in B) / n1 and m.coverage == sum(a > 0 for a in A) / n1


def test_reference_refuses_what_the_library_refuses():
    x = np.zeros((4, 3))
    for k in (0, 17):
        with pytest.raises(ValueError, match="outside"):
            R.exact(x, x, k)
    with pytest.raises(ValueError, match="k \\+ 1"):
        R.exact(x, x, 4)
    R.exact(x, x, 3)                            # n = k + 1 is legal


@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_decides_less_or_equal_and_is_not_trivial(case):
    n1, n2, D, k = case
    x, y = R.exact_case(case)
    assert x.shape == (n1, D) and y.shape == (n2, D) and x.dtype == np.float32 and set(np.unique(x)) <= {0.0, 1.0, 2.0, 3.0}
    r = R.exact(x, y, k)
    assert int(r.A.sum()) == int(r.C.sum())
    if n1 > 8:
        assert np.array_equal(x[3], x[1]) and np.array_equal(y[5], x[1]) and r.dxy[1, 5] == 0 and r.dxy[3, 5] == 0
    if n1 >= 4:
        assert 4 <= R.ties(r) <= 195             # pairs with d2 == radius: `<` in place of `<=` changes a count
        lt = R.counts_of(r.dxy, r.radii_x - 1, r.radii_y - 1)        # integers: d2 <= radius - 1 is d2 < radius
        assert any(not np.array_equal(a, b) for a, b in zip(lt, (r.A, r.B, r.C)))
    m = R.metrics(r.A, r.B, r.C, k)
    assert min(m.precision, m.recall, m.coverage) >= 0.48 and m.density > 0
    if case == (64, 65, 32, 1):
        assert (r.radii_x == 0).sum() >= 2       # the duplicate rows 1 and 3: radius 0
    # the longdouble path agrees bit for bit on integers
    q = R.real(x, y, k)
    assert np.array_equal(q.radii_x, r.radii_x) and np.array_equal(q.radii_y, r.radii_y)
    assert np.array_equal(q.A, r.A) and np.array_equal(q.B, r.B) and np.array_equal(q.C, r.C)


@pytest.mark.parametrize("case", R.REAL_CASES, ids=lambda c: "n%dx%d_k%d" % c)
def test_real_cases_keep_every_comparison_away_from_the_bound(case):
    x, y = R.real_case(case)
    r = R.real(x, y, case[2])
    b = R.bound(x, y, R.REAL_D)
    assert 1e-9 < b < 3e-9 and R.smallest_margin(r) > 1e-3 > b
    assert (r.A == 0).any() and (r.A > 0).any() and (r.C == 0).any() and (r.C > 0).any()


def test_workspace_and_argument_errors_are_reported_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    W = lib.wu_prdc_workspace_bytes
    # doubles: the norms of a bank and, per row, split and list entry, one more; the counts pass needs n1 + n2
    assert W(2, 2, 1, 0) == (2 + 2 * 1 * 2) * 8                      # one tile: one split
    assert W(2, 2, 1, 3) == (2 + 2 * 3 * 2) * 8                      # forced splits are taken as given
    assert W(130, 70, 5, 3) == (130 + 130 * 3 * 6) * 8
    assert W(70, 130, 5, 3) == W(130, 70, 5, 3)
    assert W(500, 500, 5, 0) == (500 + 500 * 8 * 6) * 8              # the test split: one split per column tile
    assert W(50000, 50000, 5, 0) == (50000 + 50000 * 1 * 6) * 8      # 782 row tiles fill the chip without splitting
    for bad in ((1, 2, 1, 0), (2, 1, 1, 0), (16, 40, 16, 0), (40, 40, 0, 0), (40, 40, 17, 0), (40, 40, 5, -1), (40, 40, 5, 1025),
                ((1 << 21) + 1, 40, 5, 0)):
        assert W(*bad) == 0, bad
    p = 64       # any non-NULL address: every call below is refused before a launch

    def radii(x=p, ldx=8, n=10, D=8, k=3, cs=0, ws=p, out=p):
        return lib.wu_knn_radii(x, ldx, n, D, k, cs, ws, out, None)

    for kwargs, word in ((dict(k=0), b"k 0 outside 1..16"), (dict(k=17), b"k 17"), (dict(n=3), b"n 3 rows, need at least k + 1 = 4"),
                         (dict(n=(1 << 21) + 1), b"over"), (dict(ldx=7), b"ldx 7"), (dict(D=0), b"D 0"), (dict(cs=-1), b"col_splits -1"),
                         (dict(cs=1025), b"col_splits 1025"), (dict(x=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(out=None), b"NULL")):
        assert radii(**kwargs) < 0, kwargs
        assert word in lib.wu_last_error(), (kwargs, lib.wu_last_error())

    def counts(x=p, ldx=8, n1=10, rx=p, y=p, ldy=8, n2=12, ry=p, D=8, ws=p, A=p, B=p, C=p):
        return lib.wu_prdc_counts(x, ldx, n1, rx, y, ldy, n2, ry, D, ws, A, B, C, None)

    for kwargs, word in ((dict(n1=0), b"n1 0"), (dict(n2=0), b"n2 0"), (dict(ldx=7), b"ldx 7"), (dict(ldy=7), b"ldy 7"), (dict(D=0), b"D 0"),
                         (dict(x=None), b"NULL"), (dict(ry=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(C=None), b"NULL")):
        assert counts(**kwargs) < 0, kwargs
        assert word in lib.wu_last_error(), (kwargs, lib.wu_last_error())


def test_wrapper_validates_on_host_tensors():
    import torch
    from wu import prdc
    x = torch.zeros(8, 3)
    for fn in (lambda: prdc.knn_radii(x, 3), lambda: prdc.manifold_counts(x, x, 3), lambda: prdc.precision_recall_density_coverage(x, x)):
        with pytest.raises(ValueError, match="CUDA"):            # no host fallback
            fn()
    with pytest.raises(ValueError, match="CUDA"):
        prdc.knn_radii(x.numpy(), 3)
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="1..16"):
            prdc.knn_radii(x, k)
        with pytest.raises(ValueError, match="1..16"):
            prdc.precision_recall_density_coverage(x, x, k=k)
    for cs in (-1, 1025):
        with pytest.raises(ValueError, match="col_splits"):
            prdc.manifold_counts(x, x, 3, col_splits=cs)
    assert prdc.PRDC._fields == ("precision", "recall", "density", "coverage")
    m = prdc.metrics_from_counts(np.array([0, 2, 1]), np.array([1, 1, 0]), np.array([3, 0]), 3)
    assert m == prdc.PRDC(0.5, 2 / 3, 3 / 6, 2 / 3) and all(isinstance(v, float) for v in m)
