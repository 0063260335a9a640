"""Top-k nearest-neighbour retrieval on the GPU (csrc/nn_topk.hip through the C ABI and through wu.retrieval) against tests/_nn_ref.py.

Exact grid: integer features in {0..3}, so every d^2 is an exact integer in fp64 whatever the order of summation -- dist2 and index must
EQUAL the int64 oracle bit for bit, at nb == k, across the 64-row tile edge, with a K-chunk tail, three column tiles, k = 16 and a bank
queried against itself, for col_splits 0 (the library's choice), 1, 2 and 3 (whole tiles, a ragged split, an empty one), on contiguous
uploads and on views of wider, longer NaN-filled buffers.  Ties are dense there (tests/test_nn_cpu.py counts them: 47 of 70 rows tie inside
their top 6, 9 of 17 exactly across the k = 16 boundary), so the index rule is decided here; one case plants three identical bank rows in
three tiles.
Real features (D = 2048): the reference's smallest gap between consecutive entries of any row's top k + 1 exceeds twice the rounding bound
4 (D + 2) 2^-53 (max|q|^2 + max|b|^2) on one d^2 (_prdc_ref.bound: derived, not measured; checked here, a violation fails), so index must
equal the reference's and dist2 lie within the bound.
Cross-check: the k-th entry of a bank against itself is wu.prdc.knn_radii bit for bit."""
import functools
import json

import numpy as np
import pytest
import torch

import _nn_ref as N
import _prdc_ref as P
from _padded_rows import padded as _padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _exact(case):
    q, b = N.exact_case(case)
    return q, b, N.exact(q, b, case[3], 0 if case[4] else -1)


@functools.lru_cache(maxsize=None)
def _three():
    q, b, k = N.three_copies_case()
    return q, b, k, N.exact(q, b, k)


@functools.lru_cache(maxsize=None)
def _real(pc):
    x, y = P.real_case(pc)
    return x, y, P.bound(x, y, P.REAL_D)


def _abi(q, b, k, self_offset, col_splits):
    """wu_nn_topk called directly on contiguous uploads; workspace and outputs start poisoned.  q is b: one upload serves both."""
    from wu import _lib
    lib = _lib.load()
    (nq, D), nb = q.shape, b.shape[0]
    bd = torch.from_numpy(b).to(DEV)
    qd = bd if q is b else torch.from_numpy(q).to(DEV)
    nbytes = lib.wu_nn_workspace_bytes(nq, nb, k, col_splits)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)          # NaN doubles, negative indices
    dist2 = torch.full((nq, k), NAN, dtype=torch.float64, device=DEV)
    index = torch.full((nq, k), -7, dtype=torch.int32, device=DEV)
    _lib.call("wu_nn_topk", qd.data_ptr(), qd.stride(0), nq, bd.data_ptr(), bd.stride(0), nb, D, k, self_offset, col_splits, ws.data_ptr(),
              nbytes, dist2.data_ptr(), index.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dist2.cpu().numpy(), index.cpu().numpy()


def _assert_equal(got, ref, what):
    (gd, gi), (rd, ri) = got, ref
    assert gd.dtype == np.float64 and gd.shape == rd.shape and gi.shape == ri.shape, what
    bad = np.argwhere(gi.astype(np.int64) != ri)
    assert bad.size == 0, f"{what}: index differs at {bad[:6].tolist()}: got {gi[tuple(bad[:6].T)]}, want {ri[tuple(bad[:6].T)]}"
    bad = np.argwhere(gd != rd.astype(np.float64))
    assert bad.size == 0, f"{what}: dist2 differs at {bad[:6].tolist()}: got {gd[tuple(bad[:6].T)]}, want {rd[tuple(bad[:6].T)]}"


def _host(out):
    assert out[0].dtype == torch.float64 and out[1].dtype == torch.int64 and out[0].is_cuda and out[1].is_cuda
    return out[0].cpu().numpy(), out[1].cpu().numpy()


@pytest.mark.parametrize("col_splits", N.COL_SPLITS)
@pytest.mark.parametrize("case", N.EXACT_GRID, ids=N.exact_case_id)
def test_exact_grid_c_abi(case, col_splits):
    q, b, ref = _exact(case)
    _assert_equal(_abi(q, b, case[3], 0 if case[4] else -1, col_splits), ref, f"abi splits {col_splits}")


@pytest.mark.parametrize("col_splits", N.COL_SPLITS)
@pytest.mark.parametrize("case", N.EXACT_GRID, ids=N.exact_case_id)
def test_exact_grid_topk_strided_and_poisoned(case, col_splits):
    """Through wu.retrieval.topk, the rows as views of wider and longer buffers: ld > D with NaN padding columns, NaN rows after nq / nb
    (one NaN read into a d^2 would become a 0 and a nearest neighbour)."""
    from wu import retrieval
    nq, nb, D, k, self_ = case
    q, b, ref = _exact(case)
    fb = _padded(b, D + 5, 1)
    fq = fb if self_ else _padded(q, D + 3, 2)
    assert fb.stride(0) == D + 5 and fq.stride(0) == (D + 5 if self_ else D + 3)
    _assert_equal(_host(retrieval.topk(fq, fb, k, exclude_self=self_, col_splits=col_splits)), ref, f"topk splits {col_splits}")


@pytest.mark.parametrize("col_splits", N.COL_SPLITS)
def test_identical_bank_rows_in_three_tiles_are_resolved_by_index(col_splits):
    from wu import retrieval
    q, b, k, ref = _three()
    assert ref[1][2].tolist() == [0, 64]
    _assert_equal(_abi(q, b, k, -1, col_splits), ref, f"abi splits {col_splits}")
    _assert_equal(_host(retrieval.topk(_padded(q, 12, 1), _padded(b, 11, 3), k, col_splits=col_splits)), ref, f"topk splits {col_splits}")


@pytest.mark.parametrize("rows", (1, 64, 100))
def test_query_chunks_give_the_bytes_of_one_call(rows):
    from wu import retrieval
    case = N.EXACT_GRID[-1]
    assert case[4]
    _, b, ref = _exact(case)
    f = _padded(b, case[2] + 1, 1)
    whole = _host(retrieval.topk(f, f, case[3], exclude_self=True))
    parts = _host(retrieval.topk(f, f, case[3], exclude_self=True, max_query_rows=rows))
    assert all(u.tobytes() == v.tobytes() for u, v in zip(whole, parts))
    _assert_equal(parts, ref, f"max_query_rows {rows}")
    # and without a self column: the chunks of (70, 130, 70, 5)
    q, b2, ref2 = _exact(N.EXACT_GRID[4])
    _assert_equal(_host(retrieval.topk(_padded(q, 70, 0), _padded(b2, 70, 0), 5, max_query_rows=rows)), ref2, f"max_query_rows {rows}")


@pytest.mark.parametrize("own", (False, True), ids=("queries_to_bank", "bank_to_itself"))
@pytest.mark.parametrize("pc,k", N.REAL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_real_features_index_equal_and_dist2_within_the_bound(pc, k, own):
    from wu import retrieval
    x, y, bound = _real(pc)
    q, b, so = (x, x, 0) if own else (y, x, -1)
    # the condition under which the order is decided: checked, never skipped
    gap = N.smallest_gap(q, b, k, so)
    assert gap > 2 * bound, f"two reference entries lie within twice the bound {bound} of each other (gap {gap})"
    ref = N.real(q, b, k, so)
    fb = _padded(b, P.REAL_D + 8, 1)
    fq = fb if own else _padded(q, P.REAL_D, 1)
    runs = (("abi", _abi(q, b, k, so, 0)), ("abi splits 2", _abi(q, b, k, so, 2)),
            ("topk", _host(retrieval.topk(fq, fb, k, exclude_self=own))),
            ("topk chunks of 50", _host(retrieval.topk(fq, fb, k, exclude_self=own, max_query_rows=50))))
    for name, (gd, gi) in runs:
        err = float(np.abs(gd - ref[0]).max())
        print(f"{pc} k {k} {'self' if own else 'q->b'} {name}: max |dist2 - ref| {err:.3e}, bound {bound:.3e}, smallest gap {gap:.3e}")
        assert np.array_equal(gi.astype(np.int64), ref[1]), f"{name}: index differs from the reference"
        assert err <= bound, f"{name}: |dist2 - ref| {err} over the bound {bound}"
        assert (np.diff(gd, axis=1) >= 0).all()
    assert all(runs[0][1][0].tobytes() == r[1][0].tobytes() for r in runs[1:])                 # one set of bytes by every route


def test_kth_entry_of_a_bank_against_itself_is_the_prdc_radius():
    """Both are the k-th smallest d^2 to another row; equal bits only if norms, d^2 and tile are formed as csrc/prdc.hip forms them."""
    from wu import prdc, retrieval
    exact = torch.from_numpy(_exact(N.EXACT_GRID[-1])[1]).to(DEV)
    real = torch.from_numpy(_real(N.REAL_CASES[0][0])[0]).to(DEV)
    for name, x, ks in (("exact", exact, (1, 5, 16)), ("real", real, (3, 8))):
        for k in ks:
            d2, _ = retrieval.topk(x, x, k, exclude_self=True)
            radii = prdc.knn_radii(x, k)
            assert d2[:, k - 1].cpu().numpy().tobytes() == radii.cpu().numpy().tobytes(), f"{name} k {k}"
    assert (retrieval.topk(exact, exact, 1, exclude_self=True)[0] == 0).sum() >= 2           # the duplicate rows 1 and 3


def test_two_runs_give_identical_bytes():
    x, y, _ = _real(N.REAL_CASES[0][0])
    a, b = _abi(y, x, 8, -1, 0), _abi(y, x, 8, -1, 0)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    c = _abi(y, x, 8, -1, 3)                        # nor do they depend on the split
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, c))


def test_wrapper_raises_value_errors():
    from wu import retrieval
    x = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError, match="topk: the bank has n = 6 rows, k = 7 needs at least k = 7 \\(n is never clamped\\)"):
        retrieval.topk(x, x, 7)
    with pytest.raises(ValueError, match="topk: the bank has n = 6 rows, k = 6 needs at least k \\+ 1 = 7"):
        retrieval.topk(x, x, 6, exclude_self=True)
    for k in (0, 17):
        with pytest.raises(ValueError, match="topk: k = .* 1..16"):
            retrieval.topk(x, x, k)
    with pytest.raises(ValueError, match="topk: feature widths 8 / 7"):
        retrieval.topk(x, x[:, :7], 3)
    with pytest.raises(ValueError, match="CUDA"):
        retrieval.topk(x, x.cpu(), 3)
    with pytest.raises(ValueError, match="unit column stride"):
        retrieval.topk(x.t(), x.t(), 3)
    with pytest.raises(ValueError, match="topk: exclude_self needs query and bank to be the same rows"):
        retrieval.topk(x[:3], x, 3, exclude_self=True)
    with pytest.raises(ValueError, match="topk: exclude_self"):
        retrieval.topk(x.clone(), x, 3, exclude_self=True)
    with pytest.raises(ValueError, match="topk: no query rows"):
        retrieval.topk(x[:0], x, 3)
    for rows in (0, -1, 2.5):
        with pytest.raises(ValueError, match="topk: max_query_rows"):
            retrieval.topk(x, x, 3, max_query_rows=rows)
    d2, idx = retrieval.topk(x, x, 6)                              # nb == k, all rows equal: every d^2 is 0, the indices ascend
    assert d2.cpu().tolist() == [[0.0] * 6] * 6 and idx.cpu().tolist() == [list(range(6))] * 6
    d2, idx = retrieval.topk(x, x, 5, exclude_self=True)           # nb == k + 1: every other row
    assert idx.cpu().tolist() == [[j for j in range(6) if j != i] for i in range(6)]


def test_nearest_report_on_the_gpu_is_plain_and_consistent():
    from wu import kid, retrieval
    x, y, _ = _real(N.REAL_CASES[1][0])
    bank, query = kid.FeatureBank(), kid.FeatureBank()
    bank.append(torch.from_numpy(x).to(DEV))
    query.append(torch.from_numpy(y).to(DEV))
    d2, idx = _host(retrieval.topk(query, bank, 1))
    rep = retrieval.nearest_report(query, bank, threshold=float(np.sqrt(np.median(d2))))
    json.loads(json.dumps(rep))
    assert rep["n_query"] == 133 and rep["n_bank"] == 70 and rep["k"] == 1
    assert rep["nearest_index"] == idx[:, 0].tolist() and rep["nearest_distance"] == np.sqrt(d2[:, 0]).tolist()
    assert rep["n_under_threshold"] == 66 and [t[2] for t in rep["under_threshold"]] == sorted(np.sqrt(d2[:, 0]).tolist())[:66]
    own = retrieval.nearest_report(bank, bank, exclude_self=True, k=3)
    assert all(i != j for i, j in enumerate(own["nearest_index"])) and len(own["neighbour_index"][0]) == 3


def test_cli_prints_nn_after_fid_from_feature_npz(tmp_path, capsys):
    """`python -m wu.fid A.npz B.npz --nn K [--nn-threshold T] [--nn-report out.json]`: the rows of B against the bank of A; without --nn
    the output is what it was."""
    from wu import fid
    D, k = 8, 4
    rng = np.random.RandomState(12)
    x = rng.rand(40, D).astype(np.float32)
    y = np.abs(x[rng.randint(0, 40, 33)] + np.exp(rng.uniform(np.log(0.02), np.log(0.8), 33))[:, None] * rng.randn(33, D)).astype(np.float32)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    for path, rows in ((pa, x), (pb, y)):
        np.savez(path, features=rows, mu=rows.astype(np.float64).mean(axis=0), sigma=np.cov(rows.astype(np.float64), rowvar=False))
    bound = P.bound(y, x, D)
    assert N.smallest_gap(y, x, k) > 2 * bound                     # the order is decided
    ref_d2, ref_i = N.real(y, x, k)
    near = np.sort(np.sqrt(ref_d2[:, 0].astype(np.float64)))
    T = float((near[9] + near[10]) / 2)                            # ten rows under it, the next one far from it in units of the bound
    assert near[10] ** 2 - T ** 2 > 2 * bound and T ** 2 - near[9] ** 2 > 2 * bound
    assert np.diff(near ** 2).min() > 2 * bound                    # and so is the order of the rows by nearest distance
    base = [pa, pb, "--weights", "unused.pth"]

    def run(extra):
        assert fid.main(base + extra) == 0
        return capsys.readouterr().out.strip().splitlines()

    plain = run([])
    assert len(plain) == 1 and plain[0].startswith("FID: ")
    lines = run(["--nn", str(k)])
    assert len(lines) == 2 and lines[0] == plain[0]
    words = lines[1].split()
    assert words[0] == "NN:" and words[1::2] == ["k", "median", "min"] and words[2] == str(k) and len(words) == 7
    # sqrt is monotone: the median and the minimum of the distances are those of d^2, each within the bound of the reference's
    assert abs(float(words[4]) ** 2 - float(np.median(ref_d2[:, 0]))) <= 2 * bound
    assert abs(float(words[6]) ** 2 - float(ref_d2[:, 0].min())) <= 2 * bound
    out = str(tmp_path / "nn.json")
    with_t = run(["--prdc", "--nn", str(k), "--nn-threshold", repr(T), "--nn-report", out])
    assert len(with_t) == 3 and with_t[0] == plain[0] and with_t[1].startswith("PRDC: ")
    assert with_t[2] == lines[1] + f" under {T}: 10"
    with open(out) as fh:
        rep = json.load(fh)
    assert rep["n_query"] == 33 and rep["n_bank"] == 40 and rep["k"] == k and rep["neighbour_index"] == ref_i.tolist()
    assert rep["n_under_threshold"] == 10 and [t[0] for t in rep["under_threshold"]] == np.argsort(ref_d2[:, 0], kind="stable")[:10].tolist()
    np.savez(str(tmp_path / "c.npz"), mu=np.zeros(D), sigma=np.eye(D))
    with pytest.raises(ValueError, match="features"):
        fid.main([pa, str(tmp_path / "c.npz"), "--weights", "unused.pth", "--nn", "1"])


def _blocks(rng):
    """A 32 x 32 image of 8 x 8 blocks of random colours."""
    return np.kron(rng.randint(0, 256, (4, 4, 3)), np.ones((8, 8, 1))).astype(np.uint8)


def test_figure_shows_a_planted_duplicate_beside_its_query(tmp_path, capsys):
    """`python -m wu.retrieval QUERY_DIR BANK_DIR --figure ...` on a handful of 32 x 32 files: the file decodes, the planted copy is the
    first row's query and the bank file it copies sits in column 1 of that row; `--self` finds the duplicate inside the bank.  The
    threshold 0.1 separates the two kinds of pair by orders of magnitude: the 64 features of the He-initialised first block are O(1) and
    every pair of different images here lies 0.52 or more apart in the float64 restatement (tests/_inception_ref.py), a copy at rounding
    error."""
    from PIL import Image
    import _inception_ref as IR
    from wu import retrieval
    rng = np.random.RandomState(5)
    bank = [_blocks(rng) for _ in range(6)]
    query = [_blocks(rng) for _ in range(4)]
    query[2] = bank[4].copy()                      # the memorised photograph
    bank[5] = bank[1].copy()                       # a re-upload inside the bank
    dirs = []
    for name, images in (("query", query), ("bank", bank)):
        d = tmp_path / name
        d.mkdir()
        for i, im in enumerate(images):
            Image.fromarray(im).save(d / f"{name}_{i:02d}.png")
        dirs.append(str(d))
    weights = str(tmp_path / "weights.pth")
    torch.save(IR.make_params(True, seed=6), weights)
    fig, out = str(tmp_path / "fig.png"), str(tmp_path / "nn.json")
    k, rows, cell, pad = 3, 2, 32, 2
    assert retrieval.main(dirs + ["--weights", weights, "--dims", "64", "--k", str(k), "--rows", str(rows), "--cell", str(cell),
                                  "--figure", fig, "--report", out, "--threshold", "0.1"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith(f"NN: k {k} median ") and line.endswith(" under 0.1: 1")
    with open(out) as fh:
        rep = json.load(fh)
    assert rep["nearest_name"][2] == "bank_04.png" and rep["query_name"][2] == "query_02.png"
    assert rep["under_threshold"][0][:2] == ["query_02.png", "bank_04.png"] and rep["n_under_threshold"] == 1
    assert int(np.argmin(rep["nearest_distance"])) == 2
    img = np.asarray(Image.open(fig).convert("RGB"))
    assert img.shape == (rows * (cell + pad) + pad, (k + 1) * (cell + pad) + pad, 3)

    def cell_at(r, c):
        y0, x0 = pad + r * (cell + pad), pad + c * (cell + pad)
        return img[y0:y0 + cell, x0:x0 + cell]

    assert np.array_equal(cell_at(0, 0), query[2]) and np.array_equal(cell_at(0, 1), bank[4])
    second = retrieval.figure_rows(np.asarray(rep["nearest_distance"])[:, None] ** 2, 2)[1]
    assert np.array_equal(cell_at(1, 0), query[second]) and np.array_equal(cell_at(1, 1), bank[rep["nearest_index"][second]])
    assert (img[:pad] == 255).all()                # the border is white

    assert retrieval.main([dirs[1], "--self", "--weights", weights, "--dims", "64", "--k", "2", "--report", out, "--threshold", "0.1"]) == 0
    with open(out) as fh:
        own = json.load(fh)
    assert own["exclude_self"] is True and own["nearest_index"][1] == 5 and own["nearest_index"][5] == 1
    assert own["under_threshold"] == [["bank_01.png", "bank_05.png", own["nearest_distance"][1]],
                                      ["bank_05.png", "bank_01.png", own["nearest_distance"][5]]]
