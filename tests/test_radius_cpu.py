"""CPU: the radius join and the ball scores without a GPU -- the numpy restatement (tests/_radius_ref.py) against literal double loops on
tiny inputs, the conditions on the case lists the GPU test relies on (checked here; a violation fails), the workspace sizes and the
argument errors of the C entry points, the validation of wu.retrieval on host tensors, and groups_from_pairs / score_report on hand-made
inputs.  No compute is launched here.

The conditions, for every case of the exact grid with more than 64 pairs: at a middle radius the join is neither empty nor everything, some
d2 equals the radius exactly (`<=` against `<` is decided), some row is empty at the len // 20 radius, and over k in {1, 3} some row has an
infinite realism and some row a rarity tie.  Two of the conditions hold in four of the five such cases and not in the 17 x 150 one, which is
asserted as it is: each of its 17 rows has three or more pairs at the len // 20 radius (its empty rows come at radius 0, 15 of 17), and
none of its rows meets two equal largest quotients at any k from 1 to 16, so it shows no realism tie.  The tie rule on three column tiles
is decided on the 70 x 130 and 129 x 129 cases."""
import json

import numpy as np
import pytest

import _nn_ref as N
import _prdc_ref as P
import _radius_ref as R


def _d2(u, v):
    return max((sum(x * x for x in u) + sum(x * x for x in v)) - 2 * sum(x * y for x, y in zip(u, v)), 0)


def _brute_join(q, b, radius2, self_offset=-1, upper_only=False):
    ptr, idx, d2 = [0], [], []
    for i, u in enumerate(q):
        for c, v in enumerate(b):
            if self_offset >= 0 and (c == self_offset + i or (upper_only and c < self_offset + i)):
                continue
            if _d2(u, v) <= radius2:
                idx.append(c)
                d2.append(_d2(u, v))
        ptr.append(len(idx))
    return ptr, idx, d2


def _brute_ball(q, b, r2, self_offset=-1):
    out = []
    for i, u in enumerate(q):
        cnt, rar, rar_i, best, arg = 0, float("inf"), -1, None, None
        for c, v in enumerate(b):
            if c == self_offset + i and self_offset >= 0:
                continue
            d = _d2(u, v)
            if d <= r2[c]:
                cnt += 1
                if r2[c] < rar:
                    rar, rar_i = r2[c], c
            rho = float("inf") if d == 0 else float(r2[c]) / float(d)
            if best is None or rho > best:
                best, arg = rho, (r2[c], d, c)
        out.append((cnt, rar, rar_i) + arg)
    return out


@pytest.mark.parametrize("nq,nb,D,self_offset,upper", [(1, 1, 1, -1, False), (3, 4, 2, -1, False), (5, 7, 2, -1, False), (6, 6, 3, 0, False),
                                                       (6, 6, 2, 0, True), (3, 9, 2, 4, False), (3, 9, 2, 4, True)])
def test_integer_oracle_agrees_with_literal_loops(nq, nb, D, self_offset, upper):
    rng = np.random.RandomState(10 * nq + nb)
    b = rng.randint(0, 3, (nb, D))
    q = b[self_offset:self_offset + nq].copy() if self_offset >= 0 else rng.randint(0, 3, (nq, D))
    ql, bl = [[int(v) for v in r] for r in q], [[int(v) for v in r] for r in b]
    for radius2 in (0, 1, 2, 5, 100):
        ptr, idx, d2 = R.exact(q, b, radius2, self_offset, upper)
        assert (ptr.tolist(), idx.tolist(), d2.tolist()) == _brute_join(ql, bl, radius2, self_offset, upper)
        assert ptr.dtype == np.int64 and idx.dtype == np.int64
        rp, ri, rd = R.real(q.astype(np.float32), b.astype(np.float32), radius2, self_offset, upper)
        assert np.array_equal(rp, ptr) and np.array_equal(ri, idx) and np.array_equal(rd, d2)
    if self_offset >= 0:                                               # the two halves of a self-join are each other's mirror
        full, half = R.exact(q, b, 2, self_offset), R.exact(q, b, 2, self_offset, True)
        assert len(full[1]) == 2 * len(half[1]) or nq != nb
    if nb >= 3:
        r2 = P.radii_of(R.exact_d(b, b), 1)
        ball = R.ball_of(R.exact_d(q, b), r2, self_offset)
        want = _brute_ball(ql, bl, [int(v) for v in r2], self_offset)
        got = list(zip(ball.count.tolist(), ball.rarity_r2.tolist(), ball.rarity_index.tolist(), ball.realism_r2.tolist(),
                       ball.realism_d2.tolist(), ball.realism_index.tolist()))
        assert got == want
        assert ((ball.rho >= 1) == (ball.count > 0)).all()


def test_reference_refuses_what_the_library_refuses():
    x = np.zeros((4, 3))
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius2"):
            R.exact(x, x, bad)
    with pytest.raises(ValueError, match="upper_only"):
        R.exact(x, x, 1, -1, True)
    with pytest.raises(ValueError, match="over nb"):
        R.exact(x, x, 1, 1)
    with pytest.raises(ValueError, match="self_offset -2"):
        R.exact(x, x, 1, -2)
    with pytest.raises(ValueError, match="at least 2"):
        R.ball_of(np.zeros((1, 1), dtype=np.int64), np.zeros(1), 0)
    assert R.exact(x, x, 0, 0, True)[0].tolist() == [0, 3, 5, 6, 6]


@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_is_not_trivial(case):
    q, b = R.exact_case(case)
    so = R.self_offset_of(case)
    d = R.exact_d(q, b)
    v = R.off_self(d, so)
    radii = R.exact_radii(case)
    assert radii[0] == 0 and radii[3] == v[-1] and radii == sorted(radii)
    sizes = [len(R.join_of(d, r, so)[1]) for r in radii]
    assert sizes[3] == len(v)                                          # every pair at the maximum
    if len(v) <= 64:
        if case[:2] == (2, 16):
            assert sizes[0] == 0                                       # the empty result
        return
    assert sizes[0] == 2                                               # the planted duplicates alone at radius 0
    assert 0 < sizes[1] < sizes[2] < len(v)
    assert all((v == r).sum() > 0 for r in radii[1:3])                 # `<=` against `<` is decided
    per = np.diff(R.join_of(d, radii[1], so)[0])
    assert (per == 0).any() == (case[:2] != (17, 150)) and np.diff(R.join_of(d, radii[3], so)[0]).max() >= 64
    assert (np.diff(R.join_of(d, 0, so)[0]) == 0).sum() >= d.shape[0] - 2      # rows without a hit
    if case[:3] == (70, 130, 70):
        assert sizes == [2, 461, 4672, 9100] and [(v == r).sum() for r in radii[1:3]] == [42, 133]
        assert np.diff(R.join_of(d, radii[2], so)[0]).max() >= 100     # rows with a hundred
    ok = R.allowed(d.shape[0], d.shape[1], so)
    realism_ties = infinite = rarity_ties = 0
    for k in R.BALL_KS:
        ball, r2 = R.exact_ball(q, b, k, so)
        assert ((ball.rho >= 1) == (ball.count > 0)).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(ok, np.where(d == 0, np.inf, r2[None, :].astype(np.float64) / d), -np.inf)
        realism_ties += int(((rho == ball.rho[:, None]).sum(axis=1) > 1).sum())
        infinite += int(np.isinf(ball.rho).sum())
        inside = (d <= r2[None, :]) & ok
        rarity_ties += int(((inside & (r2[None, :] == ball.rarity_r2[:, None])).sum(axis=1) > 1).sum())
        assert (ball.count == 0).any() and (ball.count > 0).any()
    assert infinite >= 1 and rarity_ties >= 1
    if case[:2] == (17, 150):
        assert realism_ties == 0                                       # the module docstring: the one case without a realism tie
    else:
        assert realism_ties >= 1


def test_three_copies_all_show_at_radius_zero():
    q, b, k = N.three_copies_case()
    assert N.exact(q, b, k)[1][2].tolist() == [0, 64]                  # what k = 2 shows
    ptr, idx, d2 = R.exact(q, b, 0)
    assert idx[ptr[2]:ptr[3]].tolist() == [0, 64, 128] and (d2 == 0).all()


@pytest.mark.parametrize("pc,side,so,radii", R.REAL_JOINS, ids=lambda v: str(v).replace(" ", ""))
def test_real_joins_are_decided(pc, side, so, radii):
    x, y = P.real_case(pc)
    bound = P.bound(x, y, P.REAL_D)
    assert 1e-9 < bound < 3e-9
    q, b = R.real_rows(pc, side)
    d = R.real_d(q, b)
    v = R.off_self(d, so)
    for radius2, share in zip(radii, (0.02, 0.25)):
        margin = R.join_margin(d, radius2, so)
        assert margin > 1e-4 > 2 * bound, f"a d2 lies within twice the bound {bound} of the radius {radius2} (margin {margin})"
        n = len(R.join_of(d, radius2, so)[1])
        assert abs(n / len(v) - share) < 0.01 and (np.diff(R.join_of(d, radius2, so)[0]) == 0).any() == (share < 0.1 or side == "y")


@pytest.mark.parametrize("pc", P.REAL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_real_ball_scores_are_decided(pc):
    """The fakes against the reals' balls.  One d2 and one radius each carry at most the bound, so a membership margin over twice the
    bound fixes the counts and a radius gap over twice the bound the rarity column; a quotient carries a relative error of at most
    bound / r2 + bound / d2 + 2^-53, so a relative gap over twice that fixes the realism column."""
    x, y = P.real_case(pc)
    bound = P.bound(x, y, P.REAL_D)
    k = R.REAL_BALL_KS[pc]
    d = R.real_d(y, x)
    ball, r2 = R.real_ball(y, x, k)
    member, realism, rarity = R.ball_margins(d, r2)
    assert member > 1e-3 > 2 * bound and rarity > 1e-3 > 2 * bound
    assert realism > 0.1 > 2 * (bound / float(r2.min()) + bound / float(d.min()) + P.U) and d.min() > 1
    assert (ball.count == 0).any() and (ball.count > 1).any() and (ball.rho < 1).any() and (ball.rho > 1).any()


def test_workspace_and_argument_errors_are_reported_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    W, B = lib.wu_nn_radius_workspace_bytes, lib.wu_nn_ball_workspace_bytes
    # join: both sides' norms (doubles), then one int64 offset per (row, split) and one for the total, then one byte per 64 x 64 tile
    # (rounded up to 8)
    assert W(1, 1, 0) == (1 + 1) * 8 + (1 + 1) * 8 + 8
    assert W(2, 16, 3) == (2 + 16) * 8 + (2 * 3 + 1) * 8 + 8           # forced splits are taken as given
    assert W(500, 500, 0) == 1000 * 8 + (500 * 8 + 1) * 8 + 64         # 8 row tiles: one split per column tile
    assert W(2500, 50000, 0) == 52500 * 8 + (2500 * 19 + 1) * 8 + 40 * 782     # 40 row tiles: 19 splits, 760 of the 768 resident workgroups
    assert W(50000, 50000, 0) == 100000 * 8 + (50000 * 8 + 1) * 8 + 611528     # 782 row tiles: 8 splits, 6256 workgroups in 9 rounds of 768
    assert W(215000, 215000, 0) == 430000 * 8 + (215000 * 8 + 1) * 8 + 3360 * 3360     # 3360 row tiles: 8 splits fill 35 rounds exactly
    assert W(1 << 21, 1 << 21, 0) == (1 << 22) * 8 + ((1 << 21) * 3 + 1) * 8 + (1 << 30)   # 32768 row tiles: 3 splits, 128 rounds exactly
    # scores: the norms and three doubles per (row, split), then three ints
    assert B(1, 1, 0) == (1 + 1 + 3) * 8 + 3 * 4
    assert B(2500, 50000, 0) == (52500 + 3 * 2500 * 19) * 8 + 3 * 2500 * 19 * 4
    for fn in (W, B):
        for bad in ((0, 5, 0), (5, 0, 0), (5, 40, -1), (5, 40, 1025), ((1 << 21) + 1, 40, 0), (5, (1 << 21) + 1, 0)):
            assert fn(*bad) == 0, bad
        assert fn(1 << 21, 1 << 21, 0) > 0
        assert fn(100, 301, 2) > fn(100, 300, 2) and fn(101, 300, 2) > fn(100, 300, 2) and fn(100, 300, 3) > fn(100, 300, 2)
    p = 64       # any non-NULL 8-aligned address: every call below is refused before a launch

    def count(q=p, ldq=8, nq=10, b=p, ldb=8, nb=12, D=8, r=1.0, so=-1, up=0, cs=0, ws=p, wsb=1 << 30, ptr=p):
        return lib.wu_nn_radius_count(q, ldq, nq, b, ldb, nb, D, r, so, up, cs, ws, wsb, ptr, None)

    def fill(q=p, ldq=8, nq=10, b=p, ldb=8, nb=12, D=8, r=1.0, so=-1, up=0, cs=0, ws=p, wsb=1 << 30, ptr=p, cap=5, col=p, d2=p):
        return lib.wu_nn_radius_fill(q, ldq, nq, b, ldb, nb, D, r, so, up, cs, ws, wsb, ptr, cap, col, d2, None)

    def ball(q=p, ldq=8, nq=10, b=p, ldb=8, nb=12, D=8, r2=p, so=-1, cs=0, ws=p, wsb=1 << 30, o=(p,) * 6):
        return lib.wu_nn_ball_scores(q, ldq, nq, b, ldb, nb, D, r2, so, cs, ws, wsb, *o, None)

    common = ((dict(nq=0), b"nq 0"), (dict(nq=(1 << 21) + 1), b"nq"), (dict(nb=0), b"nb 0"), (dict(nb=(1 << 21) + 1), b"nb"),
              (dict(so=-2), b"self_offset -2"), (dict(so=3), b"self_offset 3 + nq 10 over nb 12"), (dict(ldq=7), b"ldq 7"),
              (dict(ldb=7), b"ldb 7"), (dict(D=0), b"D 0"), (dict(cs=-1), b"col_splits -1"), (dict(cs=1025), b"col_splits 1025"),
              (dict(q=None), b"NULL"), (dict(b=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(ws=68), b"aligned"))
    join = ((dict(r=-1.0), b"radius2"), (dict(r=float("nan")), b"radius2"), (dict(r=float("inf")), b"radius2"),
            (dict(up=1), b"upper_only needs"), (dict(ptr=None), b"NULL"), (dict(wsb=W(10, 12, 0) - 1), b"workspace of"))
    for fn, name, cases in ((count, b"wu_nn_radius_count", common + join),
                            (fill, b"wu_nn_radius_fill", common + join + ((dict(cap=-1), b"capacity -1"), (dict(col=None), b"NULL output"),
                                                                          (dict(d2=None), b"NULL output"))),
                            (ball, b"wu_nn_ball_scores", common + ((dict(r2=None), b"NULL"), (dict(o=(p,) * 5 + (None,)), b"NULL"),
                                                                   (dict(nq=1, nb=1, so=0), b"need at least 2"),
                                                                   (dict(wsb=B(10, 12, 0) - 1), b"workspace of")))):
        for kwargs, word in cases:
            assert fn(**kwargs) < 0, (name, kwargs)
            err = lib.wu_last_error()
            assert word in err and name in err, (name, kwargs, err)
    # an empty result: capacity 0 launches nothing and takes NULL outputs
    assert fill(cap=0, col=None, d2=None) == 0


def test_wrapper_validates_on_host_tensors():
    import torch
    from wu import retrieval
    x = torch.zeros(8, 3)
    for fn in (lambda: retrieval.radius_join(x, x, 1.0), lambda: retrieval.leak_mask(x, x, 1.0), lambda: retrieval.duplicate_groups(x, 1.0),
               lambda: retrieval.ball_scores(x, x), lambda: retrieval.radius_join(x.numpy(), x, 1.0)):
        with pytest.raises(ValueError, match="CUDA"):                  # no host fallback
            fn()
    for bad in (-1.0, float("nan"), float("inf"), "a", None):
        with pytest.raises(ValueError, match="radius_join: radius2"):
            retrieval.radius_join(x, x, bad)
        with pytest.raises(ValueError, match="leak_mask: radius2"):
            retrieval.leak_mask(x, x, bad)
    for cs in (-1, 1025):
        with pytest.raises(ValueError, match="radius_join: col_splits"):
            retrieval.radius_join(x, x, 1.0, col_splits=cs)
        with pytest.raises(ValueError, match="ball_scores: col_splits"):
            retrieval.ball_scores(x, x, col_splits=cs)
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="ball_scores: k = .* 1..16"):
            retrieval.ball_scores(x, x, k)


def test_groups_from_hand_made_pairs():
    from wu import retrieval
    # 0-4, 4-7 chain into {0, 4, 7}; 2-3; 5 and 6 alone; 1-8 given as the upper half of a self-join
    n = 9
    pairs = {0: [4], 1: [8], 2: [3], 4: [7]}
    ptr = np.cumsum([0] + [len(pairs.get(i, [])) for i in range(n)])
    idx = np.array([c for i in range(n) for c in pairs.get(i, [])])
    labels, groups = retrieval.groups_from_pairs(n, ptr, idx)
    assert labels.dtype == np.int64 and labels.tolist() == [0, 1, 2, 2, 0, 5, 6, 0, 1]
    assert groups == [[0, 4, 7], [1, 8], [2, 3]]
    # the order of the pairs and a pair given twice change nothing: 7-4 and 4-0 as a full (mirrored) join
    full = {0: [4], 4: [0, 7], 7: [4], 1: [8], 8: [1], 2: [3], 3: [2]}
    ptr2 = np.cumsum([0] + [len(full.get(i, [])) for i in range(n)])
    idx2 = np.array([c for i in range(n) for c in full.get(i, [])])
    l2, g2 = retrieval.groups_from_pairs(n, ptr2, idx2)
    assert l2.tolist() == labels.tolist() and g2 == groups
    l0, g0 = retrieval.groups_from_pairs(3, np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert l0.tolist() == [0, 1, 2] and g0 == []
    with pytest.raises(ValueError, match="groups_from_pairs"):
        retrieval.groups_from_pairs(3, ptr, idx)
    with pytest.raises(ValueError, match="outside"):
        retrieval.groups_from_pairs(2, np.array([0, 1, 1]), np.array([5]))
    rep = retrieval.radius_report(ptr, idx, np.array([0.0, 4.0, 0.25, 1.0]), 2.0, bank_names=[f"b{j}" for j in range(n)])
    json.loads(json.dumps(rep))
    assert rep["n_pairs"] == 4 and rep["rows_with_hit"] == 4 and rep["largest_row"] == 1
    assert rep["pairs"] == [[0, "b4", 0.0], [1, "b8", 2.0], [2, "b3", 0.5], [4, "b7", 1.0]]
    assert retrieval.radius_line(rep) == "NN-radius: 2.0 pairs 4 rows 4 largest 1"


def test_score_report_from_hand_made_scores():
    from wu import retrieval
    inf = float("inf")
    s = retrieval.BallScores(realism=np.array([2.0, 0.5, inf, 0.25, 1.0]), realism_index=np.array([3, 1, 4, 0, 2]),
                             rarity=np.array([1.5, inf, 0.5, inf, 3.0]), rarity_index=np.array([3, -1, 4, -1, 2]),
                             count=np.array([2, 0, 5, 0, 1]), realism_r2=None, realism_d2=None, rarity_r2=None)
    rep = retrieval.score_report(s, m=2, k=3)
    json.loads(json.dumps(rep))                                        # plain Python, no infinity among the numbers
    assert rep["n_query"] == 5 and rep["k"] == 3 and rep["n_infinite_realism"] == 1
    assert rep["share_realism_below_1"] == 0.4 and rep["share_in_no_ball"] == 0.4
    q = rep["realism_quantiles"]
    assert (q["min"], q["median"], q["max"]) == (0.25, 0.75, 2.0) and list(q) == [n for n, _ in retrieval.QUANTILES]
    assert rep["rarity_quantiles"]["median"] == 1.5 and rep["rarity_quantiles"]["max"] == 3.0
    assert rep["lowest_realism"] == [[3, 0.25, 0], [1, 0.5, 1]] and rep["highest_rarity"] == [[4, 3.0, 2], [0, 1.5, 3]]
    assert retrieval.realism_line(rep) == "Realism: k 3 median 0.75 below-1 0.4 no-ball 0.4"
    named = retrieval.score_report(s, m=1, query_names=list("abcde"), bank_names=[f"b{j}" for j in range(5)])
    assert named["lowest_realism"] == [["d", 0.25, "b0"]] and named["highest_rarity"] == [["e", 3.0, "b2"]] and "k" not in named
    with pytest.raises(ValueError, match="score_report"):
        retrieval.score_report(s._replace(count=np.array([1, 2])))
