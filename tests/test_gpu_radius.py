"""The radius join and the per-row ball scores on the GPU (csrc/nn_radius.hip through the C ABI and through wu.retrieval) against
tests/_radius_ref.py.

Exact grid: integer features in {0..3}, so every d^2 is an exact integer in fp64 whatever the order of summation -- row_ptr, index and
dist2 must EQUAL the int64 oracle, at radius 0, at two middle radii that some d^2 hit exactly (`<=` is decided) and at the maximum (every
pair), across the 64-row tile edge, with a K-chunk tail, three column tiles and a bank joined with itself, for col_splits 0 (the library's
choice), 1, 2 and 3 (whole tiles, a ragged split, an empty one), on contiguous uploads with poisoned workspaces and outputs and on views of
wider, longer NaN-filled buffers.  The ball scores on the same grid, k in {1, 3}: count, the rarity pair and the realism triple EQUAL the
oracle (the quotient of two exact integers is one correctly rounded division on both sides); ties are there (tests/test_radius_cpu.py
checks it).
Real features (D = 2048): tests/test_radius_cpu.py asserts that no d^2 lies within twice the rounding bound of a radius it is compared
with and that the realism and rarity columns are decided by gaps far above the error, so the indices must equal the np.longdouble
reference's and every value lie within the bound."""
import functools
import json

import numpy as np
import pytest
import torch

import _nn_ref as N
import _prdc_ref as P
import _radius_ref as R
from _padded_rows import padded as _padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _exact(case):
    q, b = R.exact_case(case)
    so = R.self_offset_of(case)
    d = R.exact_d(q, b)
    radii = R.exact_radii(case)
    return q, b, so, d, radii, [R.join_of(d, r, so) for r in radii]


@functools.lru_cache(maxsize=None)
def _exact_ball(case, k):
    q, b, so, d, _, _ = _exact(case)
    nb = b.shape[0]
    r2 = P.radii_of(R.exact_d(b, b), k) if nb >= k + 1 else np.arange(nb, dtype=np.int64)       # 1 x 1: no k-NN radius exists; any radii
    return r2.astype(np.float64), R.ball_of(d, r2, so)


@functools.lru_cache(maxsize=None)
def _real(pc):
    x, y = P.real_case(pc)
    return x, y, P.bound(x, y, P.REAL_D)


def _upload(q, b):
    bd = torch.from_numpy(b).to(DEV)
    return (bd if q is b else torch.from_numpy(q).to(DEV)), bd


def _abi_join(q, b, radius2, self_offset, upper_only, col_splits):
    """wu_nn_radius_count + wu_nn_radius_fill called directly on contiguous uploads; workspace, row_ptr and outputs start poisoned, and
    the outputs are eight entries longer than the capacity passed: the tail must keep its poison."""
    from wu import _lib
    lib = _lib.load()
    (nq, D), nb = q.shape, b.shape[0]
    qd, bd = _upload(q, b)
    nbytes = lib.wu_nn_radius_workspace_bytes(nq, nb, col_splits)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    row_ptr = torch.full((nq + 1,), -7, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (qd.data_ptr(), qd.stride(0), nq, bd.data_ptr(), bd.stride(0), nb, D, float(radius2), self_offset, int(upper_only), col_splits,
            ws.data_ptr(), nbytes)
    _lib.call("wu_nn_radius_count", *args, row_ptr.data_ptr(), stream)
    total = int(row_ptr[nq].item())
    assert 0 <= total <= nq * nb
    col = torch.full((total + 8,), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((total + 8,), NAN, dtype=torch.float64, device=DEV)
    if total:
        _lib.call("wu_nn_radius_fill", *args, row_ptr.data_ptr(), total, col.data_ptr(), d2.data_ptr(), stream)
    else:
        _lib.call("wu_nn_radius_fill", *args, row_ptr.data_ptr(), 0, None, None, stream)       # capacity 0: NULL outputs
    torch.cuda.synchronize()
    assert (col[total:] == -7).all() and torch.isnan(d2[total:]).all()
    return row_ptr.cpu().numpy(), col[:total].cpu().numpy(), d2[:total].cpu().numpy()


def _assert_join(got, ref, what):
    (gp, gi, gd), (rp, ri, rd) = got, ref
    assert gp.dtype == np.int64 and gd.dtype == np.float64, what
    assert np.array_equal(gp, rp), f"{what}: row_ptr differs at {np.flatnonzero(gp != rp)[:6].tolist()}: got {gp[:8]}, want {rp[:8]}"
    assert np.array_equal(gi.astype(np.int64), ri), f"{what}: index differs at {np.flatnonzero(gi != ri)[:6].tolist()}"
    assert np.array_equal(gd, rd.astype(np.float64)), f"{what}: dist2 differs at {np.flatnonzero(gd != rd)[:6].tolist()}"


def _host(out):
    assert [t.dtype for t in out] == [torch.int64, torch.int64, torch.float64] and all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_c_abi(case, col_splits):
    q, b, so, _, radii, refs = _exact(case)
    for radius2, ref in zip(radii, refs):
        _assert_join(_abi_join(q, b, radius2, so, 0, col_splits), ref, f"abi radius2 {radius2} splits {col_splits}")


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_radius_join_strided_and_poisoned(case, col_splits):
    """Through wu.retrieval.radius_join, the rows as views of wider and longer buffers: ld > D with NaN padding columns, NaN rows after
    nq / nb.  And the d^2 of a pair is the d^2 topk gives for it, bit for bit."""
    from wu import retrieval
    nq, nb, D, _, self_ = case
    q, b, so, _, radii, refs = _exact(case)
    fb = _padded(b, D + 5, 1)
    fq = fb if self_ else _padded(q, D + 3, 2)
    for radius2, ref in zip(radii, refs):
        got = _host(retrieval.radius_join(fq, fb, radius2, exclude_self=self_, col_splits=col_splits))
        _assert_join(got, ref, f"radius_join radius2 {radius2} splits {col_splits}")
    k = min(16, nb - (1 if self_ else 0))
    td, ti = (t.cpu().numpy() for t in retrieval.topk(fq, fb, k, exclude_self=self_, col_splits=col_splits))
    gp, gi, gd = got                                                   # the maximum radius: every pair
    for i in range(nq):
        row = dict(zip(gi[gp[i]:gp[i + 1]].tolist(), gd[gp[i]:gp[i + 1]].tolist()))
        assert [row[c] for c in ti[i].tolist()] == td[i].tolist(), f"row {i}: dist2 is not topk's"


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
def test_three_identical_bank_rows_all_show_at_radius_zero(col_splits):
    """The copy k = 2 hides: bank rows 0, 64 and 128 equal query row 2, one per column tile."""
    from wu import retrieval
    q, b, k = N.three_copies_case()
    ref = R.exact(q, b, 0)
    assert ref[1][ref[0][2]:ref[0][3]].tolist() == [0, 64, 128]
    _assert_join(_abi_join(q, b, 0, -1, 0, col_splits), ref, f"abi splits {col_splits}")
    ptr, idx, d2 = _host(retrieval.radius_join(_padded(q, 12, 1), _padded(b, 11, 3), 0, col_splits=col_splits))
    _assert_join((ptr, idx, d2), ref, f"radius_join splits {col_splits}")
    assert idx[ptr[2]:ptr[3]].tolist() == [0, 64, 128]
    assert retrieval.topk(_padded(q, 12, 1), _padded(b, 11, 3), k)[1][2].tolist() == [0, 64]


def test_an_empty_result_has_zero_row_ptr_and_takes_null_outputs():
    from wu import retrieval
    case = R.EXACT_GRID[1]
    assert case[:2] == (2, 16)
    q, b, so, _, radii, refs = _exact(case)
    assert radii[0] == 0 and refs[0][0].tolist() == [0, 0, 0]
    for col_splits in R.COL_SPLITS:
        ptr, idx, d2 = _abi_join(q, b, 0, so, 0, col_splits)           # capacity 0, NULL outputs
        assert ptr.tolist() == [0, 0, 0] and idx.size == 0 and d2.size == 0
    out = _host(retrieval.radius_join(_padded(q, 6, 1), _padded(b, 7, 1), 0))
    assert out[0].tolist() == [0, 0, 0] and out[1].shape == (0,) and out[2].shape == (0,)
    assert retrieval.leak_mask(_padded(q, 6, 1), _padded(b, 7, 1), 0).tolist() == [False, False]


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
def test_unique_pairs_is_the_upper_half_of_the_self_join(col_splits):
    from wu import retrieval
    case = R.EXACT_GRID[-1]
    assert case[4]
    _, b, so, d, radii, refs = _exact(case)
    f = _padded(b, case[2] + 2, 1)
    for radius2, full in zip(radii, refs):
        ref = R.join_of(d, radius2, 0, True)
        assert len(full[1]) == 2 * len(ref[1])
        _assert_join(_abi_join(b, b, radius2, 0, 1, col_splits), ref, f"abi upper radius2 {radius2}")
        got = _host(retrieval.radius_join(f, f, radius2, unique_pairs=True, col_splits=col_splits))
        _assert_join(got, ref, f"unique_pairs radius2 {radius2}")
        rows = np.repeat(np.arange(129), np.diff(got[0]))
        assert (got[1] > rows).all()


@pytest.mark.parametrize("rows", (1, 64, 100))
def test_query_chunks_give_the_bytes_of_one_call(rows):
    from wu import retrieval
    case = R.EXACT_GRID[-1]
    _, b, _, d, radii, refs = _exact(case)
    f = _padded(b, case[2] + 1, 1)
    for kw, ref in ((dict(exclude_self=True), refs[2]), (dict(unique_pairs=True), R.join_of(d, radii[2], 0, True))):
        whole = _host(retrieval.radius_join(f, f, radii[2], **kw))
        parts = _host(retrieval.radius_join(f, f, radii[2], max_query_rows=rows, **kw))
        assert all(u.tobytes() == v.tobytes() for u, v in zip(whole, parts))
        _assert_join(parts, ref, f"max_query_rows {rows} {kw}")
    q, b2, _, _, radii2, refs2 = _exact(R.EXACT_GRID[4])               # and without a self column: the chunks of 70 x 130
    _assert_join(_host(retrieval.radius_join(_padded(q, 70, 0), _padded(b2, 70, 0), radii2[1], max_query_rows=rows)), refs2[1],
                 f"max_query_rows {rows}")
    mask = retrieval.leak_mask(_padded(q, 70, 0), _padded(b2, 70, 0), radii2[1], max_query_rows=rows)
    assert mask.dtype == torch.bool and mask.cpu().numpy().tolist() == (np.diff(refs2[1][0]) > 0).tolist()


def test_duplicate_groups_finds_planted_groups_of_2_3_and_20():
    """Identical rows spread over four row / column tiles; the group of 20 is more than k = 16 can ever show."""
    from wu import retrieval
    rng = np.random.RandomState(21)
    x = rng.randint(0, 4, (200, 16)).astype(np.float32)
    planted = [[3, 130], [10, 70, 199], sorted(rng.choice(np.setdiff1d(np.arange(200), [3, 130, 10, 70, 199]), 20, replace=False).tolist())]
    for g in planted:
        x[g[1:]] = x[g[0]]
    d = R.exact_d(x, x)
    assert len(R.join_of(d, 0, 0, True)[1]) == 1 + 3 + 190             # no chance duplicates: the planted pairs alone
    f = _padded(x, 19, 2)
    for kw in ({}, dict(col_splits=3), dict(max_query_rows=64)):
        labels, groups = retrieval.duplicate_groups(f, 0, **kw)
        assert groups == sorted(planted) and labels.dtype == np.int64 and labels.shape == (200,)
        want = np.arange(200)
        for g in planted:
            want[g] = g[0]
        assert labels.tolist() == want.tolist()
    assert max(len(g) for g in groups) == 20 > retrieval.MAX_K
    # at a radius that chains rows, the groups are the connected components of the oracle's pairs
    radius2 = int(np.sort(d[np.triu_indices(200, 1)])[260])           # 13: the 194 planted pairs and some eighty more
    labels, groups = retrieval.duplicate_groups(f, radius2)
    ref = retrieval.groups_from_pairs(200, *R.join_of(d, radius2, 0, True)[:2])
    assert labels.tolist() == ref[0].tolist() and groups == ref[1] and len(groups) >= 3


def _abi_ball(q, b, r2, self_offset, col_splits):
    from wu import _lib
    lib = _lib.load()
    (nq, D), nb = q.shape, b.shape[0]
    qd, bd = _upload(q, b)
    rd = torch.from_numpy(r2).to(DEV)
    nbytes = lib.wu_nn_ball_workspace_bytes(nq, nb, col_splits)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    f64 = [torch.full((nq,), NAN, dtype=torch.float64, device=DEV) for _ in range(3)]
    i32 = [torch.full((nq,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    _lib.call("wu_nn_ball_scores", qd.data_ptr(), qd.stride(0), nq, bd.data_ptr(), bd.stride(0), nb, D, rd.data_ptr(), self_offset, col_splits,
              ws.data_ptr(), nbytes, i32[0].data_ptr(), f64[0].data_ptr(), i32[1].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(),
              i32[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    count, rar_i, rl_i = (t.cpu().numpy().astype(np.int64) for t in i32)
    rar_r2, rl_r2, rl_d2 = (t.cpu().numpy() for t in f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(rl_d2 == 0, np.inf, rl_r2 / rl_d2)
    return R.Ball(count, rar_r2, rar_i, rl_r2, rl_d2, rl_i, rho)


def _assert_ball(got, ref, what):
    for name in R.Ball._fields:
        g, r = getattr(got, name), np.asarray(getattr(ref, name))
        bad = np.flatnonzero(g != r.astype(g.dtype))
        assert bad.size == 0, f"{what}: {name} differs at rows {bad[:6].tolist()}: got {g[bad[:6]]}, want {r[bad[:6]]}"


@pytest.mark.parametrize("col_splits", R.COL_SPLITS)
@pytest.mark.parametrize("k", R.BALL_KS)
@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_exact_grid_ball_scores(case, k, col_splits):
    """All of count, rarity (r2, index) and realism (r2, d2, index, quotient) against the integer oracle, through the C ABI and through
    wu.retrieval.ball_scores on padded views with the radii given and (where the bank has k + 1 rows) taken from wu.prdc.knn_radii."""
    from wu import retrieval
    nq, nb, D, _, self_ = case
    q, b, so, _, _, _ = _exact(case)
    r2, ref = _exact_ball(case, k)
    got = _abi_ball(q, b, r2, so, col_splits)
    _assert_ball(got, ref, f"abi k {k} splits {col_splits}")
    assert ((got.rho >= 1) == (got.count > 0)).all()
    fb = _padded(b, D + 5, 1)
    fq = fb if self_ else _padded(q, D + 3, 2)
    given = torch.from_numpy(r2).to(DEV)
    for radii in (given,) + ((None,) if nb >= k + 1 else ()):
        s = retrieval.ball_scores(fq, fb, k, bank_radii=radii, exclude_self=self_, col_splits=col_splits)
        assert [t.dtype for t in s[:5]] == [torch.float64, torch.int64, torch.float64, torch.int64, torch.int64] and all(t.is_cuda for t in s)
        h = R.Ball(*(t.cpu().numpy() for t in (s.count, s.rarity_r2, s.rarity_index, s.realism_r2, s.realism_d2, s.realism_index)), got.rho)
        _assert_ball(h, ref, f"ball_scores k {k} splits {col_splits}")
        # the scores themselves: square roots of exact quantities, formed on the device; two units in the last place cover one rounding
        # of the square root on either side
        realism, rarity = s.realism.cpu().numpy(), s.rarity.cpu().numpy()
        assert np.array_equal(np.isinf(realism), np.isinf(ref.rho)) and np.array_equal(np.isinf(rarity), ref.count == 0)
        fin = np.isfinite(ref.rho)
        assert np.allclose(realism[fin], np.sqrt(ref.rho[fin]), rtol=2.0 ** -51, atol=0)
        assert np.allclose(rarity[ref.count > 0], np.sqrt(ref.rarity_r2[ref.count > 0]), rtol=2.0 ** -51, atol=0)


@pytest.mark.parametrize("case", R.EXACT_GRID, ids=R.exact_case_id)
def test_count_is_the_prdc_membership_count_bit_for_bit(case):
    """Without a self column, count[i] is wu_prdc_counts' B[i]: the same d^2, the same `<=`."""
    from wu import _lib
    q, b, _, d, _, _ = _exact(case)
    (nq, D), nb = q.shape, b.shape[0]
    r2 = (np.arange(nb) % 7 + np.median(d)).astype(np.float64)         # any radii: the middle of the distances, a few values
    got = _abi_ball(q, b, r2, -1, 0)
    qd, bd = _upload(q, b)
    ws = torch.empty((nq + nb) * 8, dtype=torch.uint8, device=DEV)
    rx, ry = torch.zeros(nq, dtype=torch.float64, device=DEV), torch.from_numpy(r2).to(DEV)
    A, B, C = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (nq, nq, nb))
    _lib.call("wu_prdc_counts", qd.data_ptr(), qd.stride(0), nq, rx.data_ptr(), bd.data_ptr(), bd.stride(0), nb, ry.data_ptr(), D,
              ws.data_ptr(), A.data_ptr(), B.data_ptr(), C.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert got.count.astype(np.int32).tobytes() == B.cpu().numpy().tobytes()
    assert np.array_equal(got.count, R.ball_of(d, r2).count)


@pytest.mark.parametrize("pc,side,so,radii", R.REAL_JOINS, ids=lambda v: str(v).replace(" ", ""))
def test_real_features_join_index_equal_and_dist2_within_the_bound(pc, side, so, radii):
    from wu import retrieval
    x, y, bound = _real(pc)
    q, b = R.real_rows(pc, side)
    d = R.real_d(q, b)
    fb = _padded(b, P.REAL_D + 8, 1)
    fq = fb if side == "x" else _padded(q, P.REAL_D, 1)
    for radius2 in radii:
        # the condition under which the members are decided: checked, never skipped
        margin = R.join_margin(d, radius2, so)
        assert margin > 2 * bound, f"a d2 lies within twice the bound {bound} of the radius {radius2} (margin {margin})"
        ref = R.join_of(d, radius2, so)
        runs = (("abi", _abi_join(q, b, radius2, so, 0, 0)), ("abi splits 2", _abi_join(q, b, radius2, so, 0, 2)),
                ("radius_join", _host(retrieval.radius_join(fq, fb, radius2, exclude_self=side == "x"))),
                ("chunks of 50", _host(retrieval.radius_join(fq, fb, radius2, exclude_self=side == "x", max_query_rows=50))))
        for name, (gp, gi, gd) in runs:
            assert np.array_equal(gp, ref[0]) and np.array_equal(gi.astype(np.int64), ref[1]), f"{name}: members differ from the reference"
            err = float(np.abs(gd - ref[2]).max())
            print(f"{pc} {side} radius2 {radius2} {name}: {gi.size} pairs, max |dist2 - ref| {err:.3e}, bound {bound:.3e}, margin {margin:.3e}")
            assert err <= bound, f"{name}: |dist2 - ref| {err} over the bound {bound}"
        assert all(runs[0][1][j].astype(np.int64).tobytes() == r[1][j].astype(np.int64).tobytes() for r in runs[1:] for j in range(3))


@pytest.mark.parametrize("pc", P.REAL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_real_features_ball_scores_index_equal_and_values_within_the_bound(pc):
    from wu import retrieval
    x, y, bound = _real(pc)
    k = R.REAL_BALL_KS[pc]
    d = R.real_d(y, x)
    ref, r2 = R.real_ball(y, x, k)
    member, realism, rarity = R.ball_margins(d, r2)
    rel = bound / float(r2.min()) + bound / float(d.min()) + P.U       # the relative error of one quotient (tests/test_radius_cpu.py)
    assert member > 2 * bound and rarity > 2 * bound and realism > 2 * rel
    fq, fb = _padded(y, P.REAL_D, 1), _padded(x, P.REAL_D + 8, 1)
    outs = [retrieval.ball_scores(fq, fb, k, col_splits=cs) for cs in (0, 2)]
    for s in outs:
        assert np.array_equal(s.count.cpu().numpy(), ref.count)
        assert np.array_equal(s.rarity_index.cpu().numpy(), ref.rarity_index) and np.array_equal(s.realism_index.cpu().numpy(), ref.realism_index)
        inside = ref.count > 0
        errs = (np.abs(s.rarity_r2.cpu().numpy()[inside] - ref.rarity_r2[inside]).max(), np.abs(s.realism_r2.cpu().numpy() - ref.realism_r2).max(),
                np.abs(s.realism_d2.cpu().numpy() - ref.realism_d2).max())
        print(f"{pc} k {k}: max errors {[float(e) for e in errs]}, bound {bound:.3e}")
        assert all(float(e) <= bound for e in errs) and np.isinf(s.rarity_r2.cpu().numpy()[~inside]).all()
        got_rho = (s.realism.cpu().numpy() ** 2).astype(np.longdouble)
        assert float(np.abs(got_rho / ref.rho - 1).max()) <= rel + 4 * P.U             # and the square root and its square round once each
    assert all(u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() for u, v in zip(*outs))
    rep = retrieval.score_report(outs[0], m=5, k=k)
    json.loads(json.dumps(rep))
    low = np.sort(ref.rho.astype(np.float64))[:6]
    assert (np.diff(low) / low[:5]).min() > 2 * rel                    # the order of the five lowest is decided
    assert rep["share_in_no_ball"] == float((ref.count == 0).mean()) == rep["share_realism_below_1"]
    assert [t[0] for t in rep["lowest_realism"]] == np.argsort(ref.rho.astype(np.float64), kind="stable")[:5].tolist()


def test_wrapper_raises_value_errors():
    from wu import retrieval
    x = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError, match="radius_join: feature widths 8 / 7"):
        retrieval.radius_join(x, x[:, :7], 1.0)
    with pytest.raises(ValueError, match="radius_join: exclude_self needs query and bank to be the same rows"):
        retrieval.radius_join(x[:3], x, 1.0, exclude_self=True)
    with pytest.raises(ValueError, match="radius_join: unique_pairs needs"):
        retrieval.radius_join(x.clone(), x, 1.0, unique_pairs=True)
    with pytest.raises(ValueError, match="radius_join: no query rows"):
        retrieval.radius_join(x[:0], x, 1.0)
    for rows in (0, -1, 2.5):
        with pytest.raises(ValueError, match="radius_join: max_query_rows"):
            retrieval.radius_join(x, x, 1.0, max_query_rows=rows)
    with pytest.raises(ValueError, match="ball_scores: bank_radii"):
        retrieval.ball_scores(x, x, 3, bank_radii=torch.zeros(5, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="ball_scores: bank_radii"):
        retrieval.ball_scores(x, x, 3, bank_radii=torch.zeros(6, device=DEV))
    with pytest.raises(ValueError, match="k \\+ 1"):
        retrieval.ball_scores(x, x, 6)                                 # wu.prdc.knn_radii's own refusal
    ptr, idx, d2 = retrieval.radius_join(x, x, 0.0, unique_pairs=True)     # all rows equal: every pair once
    assert ptr.tolist() == [0, 5, 9, 12, 14, 15, 15] and idx.tolist() == [c for i in range(6) for c in range(i + 1, 6)] and (d2 == 0).all()
    s = retrieval.ball_scores(x, x, 2, exclude_self=True)              # every radius 0 and every d2 0: infinite realism, rarity 0
    assert s.count.tolist() == [5] * 6 and s.realism.tolist() == [INF] * 6 and s.rarity.tolist() == [0.0] * 6
    assert s.realism_index.tolist() == [1, 0, 0, 0, 0, 0] == s.rarity_index.tolist()


def test_cli_prints_nn_radius_and_realism_from_feature_npz(tmp_path, capsys):
    """`python -m wu.fid A.npz B.npz --nn-radius R [--nn-report out.json] --realism [--realism-k K] [--realism-report out.json]`: the rows
    of B against the bank of A; without the flags the output is what it was."""
    from wu import fid
    D, k = 8, 3
    rng = np.random.RandomState(12)
    x = rng.rand(40, D).astype(np.float32)
    y = np.abs(x[rng.randint(0, 40, 33)] + np.exp(rng.uniform(np.log(0.02), np.log(0.8), 33))[:, None] * rng.randn(33, D)).astype(np.float32)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    for path, rows in ((pa, x), (pb, y)):
        np.savez(path, features=rows, mu=rows.astype(np.float64).mean(axis=0), sigma=np.cov(rows.astype(np.float64), rowvar=False))
    bound = P.bound(y, x, D)
    d = R.real_d(y, x)
    v = np.sort(d.ravel()).astype(np.float64)
    T = float(np.sqrt((v[59] + v[60]) / 2))                            # sixty pairs inside, the next far from it in units of the bound
    assert v[60] - T * T > 4 * bound and T * T - v[59] > 4 * bound     # (T * T rounds once more: far below the bound)
    ref = R.join_of(d, np.longdouble(T * T))
    assert len(ref[1]) == 60
    ball, r2 = R.real_ball(y, x, k)
    member, realism, rarity = R.ball_margins(d, r2)
    assert member > 2 * bound and rarity > 2 * bound and realism > 2 * (bound / float(r2.min()) + bound / float(d.min()) + P.U)
    low = np.sort(ball.rho.astype(np.float64))[:11]
    assert (np.diff(low) / low[:10]).min() > 1e-3                      # the order of the ten lowest is decided
    base = [pa, pb, "--weights", "unused.pth"]

    def run(extra):
        assert fid.main(base + extra) == 0
        return capsys.readouterr().out.strip().splitlines()

    plain = run([])
    assert len(plain) == 1 and plain[0].startswith("FID: ")
    out, sout = str(tmp_path / "nn.json"), str(tmp_path / "realism.json")
    lines = run(["--nn-radius", repr(T), "--nn-report", out, "--realism", "--realism-k", str(k), "--realism-report", sout])
    assert len(lines) == 3 and lines[0] == plain[0]
    per = np.diff(ref[0])
    assert lines[1] == f"NN-radius: {T} pairs 60 rows {int((per > 0).sum())} largest {int(per.max())}"
    with open(out) as fh:
        rep = json.load(fh)["radius_join"]
    assert rep["n_pairs"] == 60 and [p[:2] for p in rep["pairs"]] == [[int(i), int(c)] for i, c in zip(np.repeat(np.arange(33), per), ref[1])]
    assert np.abs(np.array([p[2] for p in rep["pairs"]]) ** 2 - ref[2].astype(np.float64)).max() <= 2 * bound
    words = lines[2].split()
    assert words[0] == "Realism:" and words[1::2] == ["k", "median", "below-1", "no-ball"] and words[2] == str(k)
    share = float((ball.count == 0).mean())
    assert float(words[6]) == share == float(words[8]) and 0 < share < 1
    with open(sout) as fh:
        srep = json.load(fh)
    assert srep["n_query"] == 33 and srep["k"] == k and [t[0] for t in srep["lowest_realism"]] == np.argsort(ball.rho.astype(np.float64),
                                                                                                             kind="stable")[:10].tolist()
    both = run(["--nn", "2", "--nn-radius", repr(T), "--nn-report", out])
    assert len(both) == 3 and both[1].startswith("NN: k 2 ") and both[2] == lines[1]
    with open(out) as fh:
        rep2 = json.load(fh)
    assert rep2["k"] == 2 and rep2["radius_join"] == rep


def _blocks(rng):
    """A 32 x 32 image of 8 x 8 blocks of random colours."""
    return np.kron(rng.randint(0, 256, (4, 4, 3)), np.ones((8, 8, 1))).astype(np.uint8)


def test_cli_writes_groups_and_keep_lists_from_directories_with_planted_duplicates(tmp_path, capsys):
    """`python -m wu.retrieval DIR --self --radius R --groups .. --keep ..` and `QUERY_DIR BANK_DIR --radius R --keep ..` on a handful of
    32 x 32 files, the files and weights of tests/test_gpu_nn.py's figure test: every pair of different images lies 0.52 or more apart, a
    copy at rounding error, so the radius 0.1 separates them by orders of magnitude.  bank_01 has THREE copies: one more than --k 2
    shows."""
    from PIL import Image
    import _inception_ref as IR
    from wu import retrieval
    rng = np.random.RandomState(5)
    bank = [_blocks(rng) for _ in range(7)]
    query = [_blocks(rng) for _ in range(4)]
    query[2] = bank[4].copy()                      # the leaked photograph
    bank[5] = bank[1].copy()                       # re-uploads inside the bank
    bank[6] = bank[1].copy()
    bank[3] = bank[1].copy()
    dirs = []
    for name, images in (("query", query), ("bank", bank)):
        d = tmp_path / name
        d.mkdir()
        for i, im in enumerate(images):
            Image.fromarray(im).save(d / f"{name}_{i:02d}.png")
        dirs.append(str(d))
    weights = str(tmp_path / "weights.pth")
    torch.save(IR.make_params(True, seed=6), weights)
    groups, keep, fig = str(tmp_path / "groups.json"), str(tmp_path / "keep.txt"), str(tmp_path / "worst.png")
    common = ["--weights", weights, "--dims", "64", "--k", "2", "--radius", "0.1"]
    assert retrieval.main([dirs[1], "--self"] + common + ["--groups", groups, "--keep", keep]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("NN: k 2 ") and lines[-1] == "NN-radius: 0.1 pairs 6 rows 3 largest 3"
    with open(groups) as fh:
        assert json.load(fh) == [["bank_01.png", "bank_03.png", "bank_05.png", "bank_06.png"]]
    with open(keep) as fh:
        assert fh.read().split() == ["bank_00.png", "bank_01.png", "bank_02.png", "bank_04.png"]
    assert retrieval.main(dirs + common + ["--keep", keep, "--figure", fig, "--realism-worst", "2", "--cell", "32"]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == "NN-radius: 0.1 pairs 1 rows 1 largest 1"
    with open(keep) as fh:
        assert fh.read().split() == ["query_00.png", "query_01.png", "query_03.png"]
    img = np.asarray(Image.open(fig).convert("RGB"))
    assert img.shape == (2 * 34 + 2, 2 * 34 + 2, 3)
    shown = [i for i in range(4) if np.array_equal(img[2:34, 2:34], query[i])]
    assert len(shown) == 1 and shown[0] != 2       # the least realistic query is not the copy, which sits AT a bank row
