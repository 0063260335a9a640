"""CPU: top-k nearest-neighbour retrieval without a GPU -- the numpy restatement (tests/_nn_ref.py) against a three-line brute force on
tiny inputs with ties, the properties of the case lists the GPU test relies on (ties inside and across the top k on the exact grid, gaps on
the real features), wu_nn_workspace_bytes and the argument errors of wu_nn_topk, the validation of wu.retrieval on host tensors and
report_from_topk on hand-made (dist2, index).  No compute is launched here."""
import json

import numpy as np
import pytest

import _nn_ref as N
import _prdc_ref as P


def _brute(q, b, k, self_offset=-1):
    """Python numbers, one pair at a time; the order through sorted() on (d2, column) tuples."""
    d2 = lambda u, v: max((sum(x * x for x in u) + sum(x * x for x in v)) - 2 * sum(x * y for x, y in zip(u, v)), 0)
    rows = [sorted((d2(u, v), c) for c, v in enumerate(b) if c != self_offset + i or self_offset < 0)[:k] for i, u in enumerate(q)]
    return [[p[0] for p in r] for r in rows], [[p[1] for p in r] for r in rows]


@pytest.mark.parametrize("nq,nb,D,k,self_offset", [(1, 1, 1, 1, -1), (3, 4, 2, 4, -1), (5, 7, 2, 3, -1), (6, 6, 3, 5, 0), (3, 9, 2, 4, 4),
                                                   (4, 20, 1, 16, -1)])
def test_integer_oracle_agrees_with_a_literal_sort(nq, nb, D, k, self_offset):
    rng = np.random.RandomState(10 * nq + nb)
    b = rng.randint(0, 3, (nb, D))                 # three values in one or two dimensions: ties everywhere
    q = b[self_offset:self_offset + nq].copy() if self_offset >= 0 else rng.randint(0, 3, (nq, D))
    want_d, want_i = _brute([[int(v) for v in r] for r in q], [[int(v) for v in r] for r in b], k, self_offset)
    got_d, got_i = N.exact(q, b, k, self_offset)
    assert got_d.tolist() == want_d and got_i.tolist() == want_i and got_i.dtype == np.int64
    if nb > k + 1:
        assert N.ties_inside(q, b, k, self_offset) > 0             # the index rule is exercised
    if self_offset >= 0:
        assert all(self_offset + i not in row for i, row in enumerate(want_i))
    # the longdouble path on the same integers gives the same numbers
    real_d, real_i = N.real(q.astype(np.float32), b.astype(np.float32), k, self_offset)
    assert np.array_equal(real_d, got_d) and np.array_equal(real_i, got_i)


def test_real_restatement_agrees_with_a_literal_sort():
    rng = np.random.RandomState(3)
    q, b, k = rng.rand(6, 5).astype(np.float32), rng.rand(11, 5).astype(np.float32), 4
    want_d, want_i = _brute([[float(v) for v in r] for r in q], [[float(v) for v in r] for r in b], k)
    got_d, got_i = N.real(q, b, k)
    assert N.smallest_gap(q, b, k) > 1e-9          # float64 loops against longdouble matrices cannot disagree on the order
    assert got_i.tolist() == want_i
    np.testing.assert_allclose(got_d.astype(np.float64), want_d, rtol=0, atol=1e-13)


def test_reference_refuses_what_the_library_refuses():
    x = np.zeros((4, 3))
    for k in (0, 17):
        with pytest.raises(ValueError, match="outside"):
            N.exact(x, x, k)
    with pytest.raises(ValueError, match="needs k$"):
        N.exact(x, x, 5)
    with pytest.raises(ValueError, match="needs k \\+ 1"):
        N.exact(x, x, 4, 0)
    with pytest.raises(ValueError, match="over nb"):
        N.exact(x, x, 2, 1)
    N.exact(x, x, 4)                                # nb == k is legal without a self column
    N.exact(x, x, 3, 0)                             # nb == k + 1 with one


def test_exact_grid_exercises_the_index_rule():
    """What the issue states about the cases, checked: ties inside the top k + 1 and across the k-th / (k + 1)-th boundary are dense."""
    shapes = {}
    for c in N.EXACT_GRID:
        nq, nb, D, k, self_ = c
        q, b = N.exact_case(c)
        assert q.shape == (nq, D) and b.shape == (nb, D) and q.dtype == np.float32 and set(np.unique(b)) <= {0.0, 1.0, 2.0, 3.0}
        shapes[c[:4]] = (q, b, 0 if self_ else -1)
    q, b, so = shapes[(70, 130, 70, 5)]
    assert N.ties_inside(q, b, 6, so) == 47 and N.ties_across(q, b, 5, so) == 21
    q, b, so = shapes[(17, 150, 33, 16)]
    assert N.ties_across(q, b, 16, so) == 9 and N.ties_inside(q, b, 16, so) == 17
    q, b, so = shapes[(129, 129, 31, 5)]
    assert so == 0 and q is b and N.ties_across(q, b, 5, so) == 40
    _, idx = N.exact(q, b, 5, 0)
    assert not (idx == np.arange(129)[:, None]).any()              # no row is its own neighbour ..
    assert idx[1, 0] == 3 and idx[3, 0] == 1                       # .. but its duplicate elsewhere in the bank is
    q, b, k = N.three_copies_case()
    d, idx = N.exact(q, b, k)
    assert np.array_equal(b[0], b[64]) and np.array_equal(b[0], b[128])
    assert idx[2].tolist() == [0, 64] and d[2].tolist() == [0, 0]  # 128 ties with both and is dropped by the index rule alone


@pytest.mark.parametrize("pc,k", N.REAL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_real_cases_keep_the_order_decided(pc, k):
    x, y = P.real_case(pc)
    bound = P.bound(x, y, P.REAL_D)
    assert 1e-9 < bound < 3e-9
    for q, b, so in ((y, x, -1), (x, x, 0)):
        assert N.smallest_gap(q, b, k, so) > 3e-4 > 2 * bound


def test_workspace_and_argument_errors_are_reported_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    W = lib.wu_nn_workspace_bytes
    # doubles: both sides' norms and, per query row, split and list entry, one d2; then one int per list entry
    assert W(1, 1, 1, 0) == (1 + 1 + 1) * 8 + 1 * 4
    assert W(2, 16, 16, 3) == (2 + 16 + 2 * 3 * 16) * 8 + 2 * 3 * 16 * 4        # forced splits are taken as given
    assert W(500, 500, 8, 0) == (500 + 500 + 500 * 8 * 8) * 8 + 500 * 8 * 8 * 4  # the test split: one split per column tile
    assert W(50000, 50000, 8, 0) == (100000 + 50000 * 8) * 8 + 50000 * 8 * 4     # 782 row tiles fill the chip without splitting
    assert W(215000, 215000, 8, 0) == (430000 + 215000 * 8) * 8 + 215000 * 8 * 4
    # monotone in every argument at a forced number of splits, and in nb and k when the library chooses it (the choice itself falls as
    # nq grows: a 65th query row halves the splits, so bytes are not monotone in nq there)
    base = (100, 300, 5, 2)
    for pos in range(4):
        more = list(base)
        more[pos] += 1
        assert W(*more) > W(*base), pos
    for nb in (64, 65, 4096, 4097):
        assert W(100, nb + 1, 5, 0) >= W(100, nb, 5, 0) + 8 and W(100, nb, 6, 0) > W(100, nb, 5, 0)
    for bad in ((0, 5, 1, 0), (5, 0, 1, 0), (5, 4, 5, 0), (5, 40, 0, 0), (5, 40, 17, 0), (5, 40, 5, -1), (5, 40, 5, 1025),
                ((1 << 21) + 1, 40, 5, 0), (5, (1 << 21) + 1, 5, 0)):
        assert W(*bad) == 0, bad
    assert W(1 << 21, 1 << 21, 16, 0) > 0
    p = 64       # any non-NULL 8-aligned address: every call below is refused before a launch

    def topk(q=p, ldq=8, nq=10, b=p, ldb=8, nb=12, D=8, k=3, so=-1, cs=0, ws=p, wsb=1 << 30, d=p, i=p):
        return lib.wu_nn_topk(q, ldq, nq, b, ldb, nb, D, k, so, cs, ws, wsb, d, i, None)

    for kwargs, word in ((dict(k=0), b"k 0 outside 1..16"), (dict(k=17), b"k 17"), (dict(nq=0), b"nq 0"), (dict(nq=(1 << 21) + 1), b"nq"),
                         (dict(nb=(1 << 21) + 1), b"over"), (dict(nb=2), b"nb 2 bank rows, need at least k = 3"),
                         (dict(nb=3, nq=3, so=0), b"need at least k + 1 = 4"), (dict(so=-2), b"self_offset -2"),
                         (dict(so=3), b"self_offset 3 + nq 10 over nb 12"), (dict(ldq=7), b"ldq 7"), (dict(ldb=7), b"ldb 7"), (dict(D=0), b"D 0"),
                         (dict(cs=-1), b"col_splits -1"), (dict(cs=1025), b"col_splits 1025"), (dict(q=None), b"NULL"), (dict(b=None), b"NULL"),
                         (dict(ws=None), b"NULL"), (dict(d=None), b"NULL"), (dict(i=None), b"NULL"), (dict(ws=68), b"aligned"),
                         (dict(wsb=W(10, 12, 3, 0) - 1), b"workspace of")):
        assert topk(**kwargs) < 0, kwargs
        assert word in lib.wu_last_error(), (kwargs, lib.wu_last_error())


def test_wrapper_validates_on_host_tensors():
    import torch
    from wu import retrieval
    x = torch.zeros(8, 3)
    for fn in (lambda: retrieval.topk(x, x, 3), lambda: retrieval.nearest_report(x, x), lambda: retrieval.topk(x.numpy(), x, 3)):
        with pytest.raises(ValueError, match="CUDA"):            # no host fallback
            fn()
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="topk: k = .* 1..16"):
            retrieval.topk(x, x, k)
    for cs in (-1, 1025):
        with pytest.raises(ValueError, match="topk: col_splits"):
            retrieval.topk(x, x, 3, col_splits=cs)


def test_report_from_hand_made_topk():
    from wu import retrieval
    d2 = np.array([[4.0, 9.0], [0.0, 1.0], [0.25, 0.25], [0.0, 16.0], [1.0, 4.0]])
    idx = np.array([[7, 2], [3, 0], [5, 6], [1, 9], [3, 4]])
    rep = retrieval.report_from_topk(d2, idx, threshold=1.0, n_bank=10)
    json.loads(json.dumps(rep))                                    # plain Python all the way down
    assert rep["n_query"] == 5 and rep["n_bank"] == 10 and rep["k"] == 2 and rep["exclude_self"] is False
    assert rep["nearest_index"] == [7, 3, 5, 1, 3] and rep["nearest_distance"] == [2.0, 0.0, 0.5, 0.0, 1.0]
    assert rep["neighbour_index"] == idx.tolist() and rep["neighbour_distance"] == np.sqrt(d2).tolist()
    qs = rep["quantiles"]
    assert (qs["min"], qs["median"], qs["max"]) == (0.0, 0.5, 2.0) and qs["p25"] == 0.0 and qs["p75"] == 1.0
    assert list(qs) == ["min", "p01", "p05", "p25", "median", "p75", "p95", "p99", "max"]
    # strictly under the threshold; by distance, then query index: the two zeros come as queries 1 and 3, then 0.5; 1.0 is not under 1.0
    assert rep["under_threshold"] == [[1, 3, 0.0], [3, 1, 0.0], [2, 5, 0.5]] and rep["n_under_threshold"] == 3
    assert retrieval.nn_line(rep) == "NN: k 2 median 0.5 min 0.0 under 1.0: 3"
    import torch
    named = retrieval.report_from_topk(torch.from_numpy(d2[:, :1]), torch.from_numpy(idx[:, :1]), 0.75, True, list("abcde"),
                                       [f"b{j}" for j in range(10)])
    assert named["k"] == 1 and "neighbour_index" not in named and named["exclude_self"] is True and "n_bank" not in named
    assert named["query_name"] == list("abcde") and named["nearest_name"] == ["b7", "b3", "b5", "b1", "b3"]
    assert named["under_threshold"] == [["b", "b3", 0.0], ["d", "b1", 0.0], ["c", "b5", 0.5]]
    plain = retrieval.report_from_topk(d2, idx)
    assert "threshold" not in plain and "under_threshold" not in plain and retrieval.nn_line(plain) == "NN: k 2 median 0.5 min 0.0"
    assert retrieval.figure_rows(d2, 3) == [1, 3, 2] and retrieval.figure_rows(d2, 99) == [1, 3, 2, 4, 0]
    with pytest.raises(ValueError, match="report_from_topk"):
        retrieval.report_from_topk(d2, idx[:, :1])
    with pytest.raises(ValueError, match="query_names"):
        retrieval.report_from_topk(d2, idx, query_names=["a"])
