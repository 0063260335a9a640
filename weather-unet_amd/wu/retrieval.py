"""Nearest-neighbour retrieval on feature rows: which rows of a bank is this row closest to, and how close?  The per-row question behind
the memorisation figure (generated images beside their nearest training photographs: does a low FID come from copying?), the leakage check
(a test photograph whose near-duplicate sits in the training set) and the search for near-duplicates inside one directory.

    dist2, index = topk(query, bank, k=8)                       # (nq, k) float64 squared distances, ascending; (nq, k) int64 bank rows
    dist2, index = topk(bank, bank, k=8, exclude_self=True)     # a bank against itself, every row's own column skipped
    report = nearest_report(query, bank, threshold=0.5)         # a JSON-serialisable dict: nearest row, distance, quantiles, pairs under 0.5

    python -m wu.retrieval QUERY_DIR BANK_DIR --weights W [--k 8] [--rows 16] [--cell 128] [--figure fig.png] [--report out.json]
    python -m wu.retrieval DIR --self --weights W ...           # near-duplicates inside one directory

Semantics, in full.  For float32 rows a, b widened to float64, ``d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0)``, every operation rounded
on its own: wu.prdc's d2, formed the same way, so ``topk(x, x, k, exclude_self=True)[0][:, k - 1]`` is ``wu.prdc.knn_radii(x, k)`` bit for
bit.  Row i of the result holds the k smallest pairs ``(d2(q_i, b_c), c)`` in the lexicographic order: the smaller d2 first, on equal d2
the smaller bank row.  The order is total, so the result is one fixed set of bytes whatever ``col_splits`` and ``max_query_rows`` are.
``exclude_self`` skips, for query row i, bank row i and nothing else: a duplicate of the row elsewhere in the bank stays (that is what a
duplicate search looks for).  1 <= k <= 16; a bank with fewer than k rows (k + 1 with ``exclude_self``) is an error, never clamped, so every
entry is a real neighbour.  A top-k search finds a duplicate unless the row has more than k copies; every pair under a radius comes from
``radius_join``:

    row_ptr, index, dist2 = radius_join(query, bank, radius2)          # CSR: row i's bank rows with d2 <= radius2, ascending
    keep = ~leak_mask(test, train, radius2)                             # the leakage-free split
    labels, groups = duplicate_groups(rows, radius2)                    # connected components of the self-join: keep one row of each
    s = ball_scores(fake, real, k=3)                                    # per-row realism (Kynkaanniemi et al. 2019) and rarity (Han et al. 2022)

    python -m wu.retrieval DIR --self --weights W --radius R [--groups groups.json] [--keep keep.txt]
    python -m wu.retrieval QUERY_DIR BANK_DIR --weights W --radius R --keep keep.txt       # the query files with no bank row inside R

The distance matrix is never stored (wu_nn_topk, csrc/nn_topk.hip: 64 x 64 tiles on the fp64 matrix cores, the tile of csrc/gram_f64.h
that the KID and PRDC share, consumed by the epilogue).  There is no host fallback."""
import argparse
import collections
import json
import sys

import numpy as np
import torch

from . import _lib
from .features import as_rows
from .layout import stream_ptr

MAX_K = 16
MAX_COL_SPLITS = 1024
QUANTILES = (("min", 0.0), ("p01", 0.01), ("p05", 0.05), ("p25", 0.25), ("median", 0.5), ("p75", 0.75), ("p95", 0.95), ("p99", 0.99),
             ("max", 1.0))


def _rows(f, who):
    f = as_rows(f, who)
    if f.shape[1] < 1:
        raise ValueError(f"{who}: feature width {f.shape[1]} must be at least 1")
    return f


def _check_k(k, col_splits, who):
    if int(k) != k or k < 1 or k > MAX_K:
        raise ValueError(f"{who}: k = {k} must be an integer in 1..{MAX_K}")
    if int(col_splits) != col_splits or col_splits < 0 or col_splits > MAX_COL_SPLITS:
        raise ValueError(f"{who}: col_splits = {col_splits} must be an integer in 0..{MAX_COL_SPLITS} (0: chosen from the sizes)")


def topk(query, bank, k, exclude_self=False, col_splits=0, max_query_rows=None):
    """(dist2, index): (nq, k) float64 squared distances, ascending, and (nq, k) int64 bank rows, both CUDA tensors (the module docstring
    has the order).  ``query`` / ``bank``: FeatureBanks or (n, D) float32 CUDA tensors with unit column stride.  ``exclude_self``: query
    and bank must be the same rows; row i's own column is skipped.  ``col_splits``: 0 lets the library split the bank's columns over
    workgroups, a positive value forces that many.  ``max_query_rows``: run the queries in chunks of that many rows (the workspace then
    scales with the chunk); the result is the same bytes.  Nothing is synchronised."""
    who = "topk"
    _check_k(k, col_splits, who)
    q, b = _rows(query, who), _rows(bank, who)
    k, col_splits = int(k), int(col_splits)
    if q.shape[1] != b.shape[1] or q.device != b.device:
        raise ValueError(f"{who}: feature widths {q.shape[1]} / {b.shape[1]} or devices differ")
    (nq, d), nb = q.shape, b.shape[0]
    if exclude_self and (q.data_ptr() != b.data_ptr() or q.shape != b.shape or q.stride() != b.stride()):
        raise ValueError(f"{who}: exclude_self needs query and bank to be the same rows (one FeatureBank or tensor passed twice)")
    need = k + 1 if exclude_self else k
    if nb < need:
        raise ValueError(f"{who}: the bank has n = {nb} rows, k = {k} needs at least {'k + 1' if exclude_self else 'k'} = {need} "
                         "(n is never clamped)")
    if nq < 1:
        raise ValueError(f"{who}: no query rows")
    chunk = nq if max_query_rows is None else max_query_rows
    if int(chunk) != chunk or chunk < 1:
        raise ValueError(f"{who}: max_query_rows = {max_query_rows} must be a positive integer or None")
    chunk = min(int(chunk), nq)
    lib = _lib.load()
    dev = q.device
    with torch.cuda.device(dev):
        dist2 = torch.empty(nq, k, dtype=torch.float64, device=dev)
        index = torch.empty(nq, k, dtype=torch.int32, device=dev)
        spaces = {}
        for r0 in range(0, nq, chunk):
            n = min(chunk, nq - r0)
            if n not in spaces:
                nbytes = lib.wu_nn_workspace_bytes(n, nb, k, col_splits)
                if nbytes == 0:
                    raise ValueError(f"{who}: nq = {n} / nb = {nb} / k = {k} / col_splits = {col_splits} out of the library's range")
                spaces[n] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ws, rows = spaces[n], q[r0:r0 + n]
            _lib.call("wu_nn_topk", rows.data_ptr(), q.stride(0), n, b.data_ptr(), b.stride(0), nb, d, k, r0 if exclude_self else -1,
                      col_splits, ws.data_ptr(), ws.numel(), dist2[r0:r0 + n].data_ptr(), index[r0:r0 + n].data_ptr(), stream_ptr())
        return dist2, index.long()


def _host(a, dtype):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(dtype)


def _name(names, i):
    return int(i) if names is None else str(names[int(i)])


def report_from_topk(dist2, index, threshold=None, exclude_self=False, query_names=None, bank_names=None, n_bank=None):
    """The dict of ``nearest_report`` from a finished ``(dist2, index)`` pair (tensors or arrays of shape (nq, k), k >= 1): pure host
    code.  Distances are ``sqrt(d2)``.  Keys: ``n_query``, ``n_bank`` (when given), ``k``, ``exclude_self``; per query row
    ``nearest_index`` / ``nearest_distance`` (and ``nearest_name`` / ``query_name`` with names); ``quantiles`` of the nearest distances
    (min, p01, p05, p25, median, p75, p95, p99, max; numpy's linear interpolation); with k > 1 ``neighbour_index`` /
    ``neighbour_distance`` (nq lists of k); with a threshold ``threshold``, ``under_threshold`` -- the ``[query, bank, distance]`` triples
    of nearest pairs with distance < threshold (names in place of indices where names are given), sorted by distance, then query
    index, then bank index -- and ``n_under_threshold``.  With ``exclude_self`` on one set of rows, a duplicate pair (i, j) shows twice,
    as (i, j) and as (j, i)."""
    d2, idx = _host(dist2, np.float64), _host(index, np.int64)
    if d2.ndim != 2 or d2.shape != idx.shape or d2.shape[1] < 1:
        raise ValueError(f"report_from_topk: dist2 {d2.shape} and index {idx.shape} must both be (nq, k), k >= 1")
    nq, k = d2.shape
    for names, n, what in ((query_names, nq, "query_names"), (bank_names, n_bank, "bank_names")):
        if names is not None and n is not None and len(names) != n:
            raise ValueError(f"report_from_topk: {len(names)} {what} for {n} rows")
    dist = np.sqrt(d2)
    near_d, near_i = dist[:, 0], idx[:, 0]
    rep = {"n_query": int(nq), "k": int(k), "exclude_self": bool(exclude_self)}
    if n_bank is not None:
        rep["n_bank"] = int(n_bank)
    rep["nearest_index"] = [int(i) for i in near_i]
    rep["nearest_distance"] = [float(v) for v in near_d]
    if query_names is not None:
        rep["query_name"] = [str(s) for s in query_names]
    if bank_names is not None:
        rep["nearest_name"] = [str(bank_names[int(i)]) for i in near_i]
    rep["quantiles"] = {name: float(np.quantile(near_d, p)) for name, p in QUANTILES} if nq else {}
    if k > 1:
        rep["neighbour_index"] = [[int(i) for i in row] for row in idx]
        rep["neighbour_distance"] = [[float(v) for v in row] for row in dist]
    if threshold is not None:
        threshold = float(threshold)
        rows = np.flatnonzero(near_d < threshold)
        rows = rows[np.lexsort((near_i[rows], rows, near_d[rows]))]
        rep["threshold"] = threshold
        rep["under_threshold"] = [[_name(query_names, i), _name(bank_names, near_i[i]), float(near_d[i])] for i in rows]
        rep["n_under_threshold"] = int(rows.size)
    return rep


def nearest_report(query, bank, threshold=None, exclude_self=False, query_names=None, bank_names=None, k=1):
    """A plain dict (JSON-serialisable) on the nearest bank row of every query row: ``report_from_topk`` of ``topk(query, bank, k,
    exclude_self)``.  ``threshold``: also list the pairs closer than it (a distance, not a squared one).  ``k`` > 1 adds every row's k
    neighbours.  Synchronises (the results are read on the host)."""
    dist2, index = topk(query, bank, k, exclude_self=exclude_self)
    return report_from_topk(dist2, index, threshold, exclude_self, query_names, bank_names, n_bank=as_rows(bank, "nearest_report").shape[0])


def nn_line(report):
    """The ``NN:`` line of ``python -m wu.fid ... --nn K`` and of this module's command line."""
    q = report["quantiles"]
    line = f"NN: k {report['k']} median {q['median']} min {q['min']}"
    if "threshold" in report:
        line += f" under {report['threshold']}: {report['n_under_threshold']}"
    return line


# ----------------------------------------------------------------------------------------------
# every pair under a radius: the leakage-free split and the duplicate groups
# ----------------------------------------------------------------------------------------------
def _check_join(radius2, col_splits, who):
    try:
        ok = float(radius2) >= 0.0 and float(radius2) != float("inf")
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: radius2 = {radius2} must be a finite number >= 0 (a SQUARED distance)")
    if int(col_splits) != col_splits or col_splits < 0 or col_splits > MAX_COL_SPLITS:
        raise ValueError(f"{who}: col_splits = {col_splits} must be an integer in 0..{MAX_COL_SPLITS} (0: chosen from the sizes)")


def _pair(query, bank, own, who):
    q, b = _rows(query, who), _rows(bank, who)
    if q.shape[1] != b.shape[1] or q.device != b.device:
        raise ValueError(f"{who}: feature widths {q.shape[1]} / {b.shape[1]} or devices differ")
    if own and (q.data_ptr() != b.data_ptr() or q.shape != b.shape or q.stride() != b.stride()):
        raise ValueError(f"{who}: {own} needs query and bank to be the same rows (one FeatureBank or tensor passed twice)")
    if q.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError(f"{who}: no {'query' if q.shape[0] < 1 else 'bank'} rows")
    return q, b


def _chunk(max_query_rows, nq, who):
    chunk = nq if max_query_rows is None else max_query_rows
    if int(chunk) != chunk or chunk < 1:
        raise ValueError(f"{who}: max_query_rows = {max_query_rows} must be a positive integer or None")
    return min(int(chunk), nq)


def _radius_passes(q, b, radius2, self_rows, upper, col_splits, chunk, fill, who):
    """The count pass per chunk of query rows and, with ``fill``, the fill pass: (row_ptr, col or None, dist2 or None).  One 8-byte read
    per chunk sizes its outputs."""
    (nq, d), nb = q.shape, b.shape[0]
    lib = _lib.load()
    dev = q.device
    with torch.cuda.device(dev):
        ptrs, cols, d2s, spaces, base = [], [], [], {}, 0
        for r0 in range(0, nq, chunk):
            n = min(chunk, nq - r0)
            if n not in spaces:
                nbytes = lib.wu_nn_radius_workspace_bytes(n, nb, col_splits)
                if nbytes == 0:
                    raise ValueError(f"{who}: nq = {n} / nb = {nb} / col_splits = {col_splits} out of the library's range")
                spaces[n] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ws, rows = spaces[n], q[r0:r0 + n]
            ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
            args = (rows.data_ptr(), q.stride(0), n, b.data_ptr(), b.stride(0), nb, d, radius2, r0 if self_rows else -1, 1 if upper else 0,
                    col_splits, ws.data_ptr(), ws.numel())
            _lib.call("wu_nn_radius_count", *args, ptr.data_ptr(), stream_ptr())
            total = int(ptr[n].item())                     # the one synchronisation: it sizes the chunk's output
            ptrs.append(ptr[:n] + base)
            base += total
            if fill:
                col = torch.empty(total, dtype=torch.int32, device=dev)
                d2 = torch.empty(total, dtype=torch.float64, device=dev)
                _lib.call("wu_nn_radius_fill", *args, ptr.data_ptr(), total, col.data_ptr() if total else None,
                          d2.data_ptr() if total else None, stream_ptr())
                cols.append(col)
                d2s.append(d2)
        ptrs.append(torch.full((1,), base, dtype=torch.int64, device=dev))
        row_ptr = torch.cat(ptrs)
        if not fill:
            return row_ptr, None, None
        return row_ptr, torch.cat(cols).long(), torch.cat(d2s)


def radius_join(query, bank, radius2, exclude_self=False, unique_pairs=False, col_splits=0, max_query_rows=None):
    """Every pair (query row i, bank row c) with ``d2(q_i, b_c) <= radius2`` (the module's d2, the same bits ``topk`` returns; ``<=`` as
    wu.prdc decides membership) in CSR form: ``(row_ptr, index, dist2)``, CUDA tensors of (nq + 1,) int64, (pairs,) int64 and (pairs,)
    float64.  Row i's bank rows are ``index[row_ptr[i]:row_ptr[i + 1]]``, ascending, their squared distances beside them.
    ``exclude_self``: query and bank are the same rows and the pair (i, i) is left out.  ``unique_pairs``: the same, and only c > i is kept
    -- each unordered pair once.  ``col_splits`` and ``max_query_rows`` as in ``topk``: the result is the same bytes whatever they are.
    The pair count is read from the device once per chunk of query rows (8 bytes) to size the output; that is the only synchronisation.
    The distance matrix is never stored (wu_nn_radius_count / wu_nn_radius_fill, csrc/nn_radius.hip)."""
    who = "radius_join"
    _check_join(radius2, col_splits, who)
    own = "unique_pairs" if unique_pairs else ("exclude_self" if exclude_self else None)
    q, b = _pair(query, bank, own, who)
    chunk = _chunk(max_query_rows, q.shape[0], who)
    return _radius_passes(q, b, float(radius2), own is not None, bool(unique_pairs), int(col_splits), chunk, True, who)


def leak_mask(query, bank, radius2, col_splits=0, max_query_rows=None):
    """(nq,) bool CUDA tensor: the query rows with at least one bank row inside the radius (``d2 <= radius2``) -- the test photographs to
    drop for a leakage-free split.  The count pass of ``radius_join`` alone: nothing is written per pair."""
    who = "leak_mask"
    _check_join(radius2, col_splits, who)
    q, b = _pair(query, bank, None, who)
    row_ptr, _, _ = _radius_passes(q, b, float(radius2), False, False, int(col_splits), _chunk(max_query_rows, q.shape[0], who), False, who)
    return row_ptr[1:] > row_ptr[:-1]


def groups_from_pairs(n, row_ptr, index):
    """Connected components of the graph on n rows whose edges are the CSR pairs: ``(labels, groups)``, pure host code (a union-find over
    the pair list; the list of a duplicate search is short).  ``labels``: (n,) int64 numpy array, every row's label the smallest row of its
    component, so it does not depend on the order of the pairs.  ``groups``: the components of two or more rows, each an ascending list
    of rows, listed by label."""
    ptr, idx = _host(row_ptr, np.int64), _host(index, np.int64)
    if ptr.shape != (n + 1,) or ptr[0] != 0 or ptr[-1] != idx.size or (np.diff(ptr) < 0).any():
        raise ValueError(f"groups_from_pairs: row_ptr {ptr.shape} does not describe {idx.size} pairs over {n} rows")
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"groups_from_pairs: a pair names a row outside 0..{n - 1}")
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    rows = np.repeat(np.arange(n), np.diff(ptr))
    for i, c in zip(rows.tolist(), idx.tolist()):
        a, b = find(i), find(c)
        if a != b:
            parent[max(a, b)] = min(a, b)          # the root is always the smallest row of its component
    labels = np.array([find(i) for i in range(n)], dtype=np.int64)
    members = {}
    for i, l in enumerate(labels.tolist()):
        members.setdefault(l, []).append(i)
    return labels, [m for _, m in sorted(members.items()) if len(m) > 1]


def duplicate_groups(rows, radius2, col_splits=0, max_query_rows=None):
    """``(labels, groups)`` of ``groups_from_pairs`` on the self-join ``radius_join(rows, rows, radius2, unique_pairs=True)``: the sets of
    near-duplicates from which one keeps a single member.  Rows chain: a and c share a group when a ~ b and b ~ c.  A group may hold any
    number of rows (a top-k search shows at most k copies).  Synchronises (the pair list is read on the host)."""
    row_ptr, index, _ = radius_join(rows, rows, radius2, unique_pairs=True, col_splits=col_splits, max_query_rows=max_query_rows)
    return groups_from_pairs(int(row_ptr.numel()) - 1, row_ptr, index)


def radius_report(row_ptr, index, dist2, radius, query_names=None, bank_names=None):
    """A plain dict on a finished ``radius_join``: ``radius`` (a distance), ``n_pairs``, ``rows_with_hit``, ``largest_row`` (the most
    pairs any query row has) and ``pairs``, the ``[query, bank, distance]`` triples in CSR order (names in place of indices where names are
    given).  Pure host code."""
    ptr, idx, d2 = _host(row_ptr, np.int64), _host(index, np.int64), _host(dist2, np.float64)
    per = np.diff(ptr)
    rows = np.repeat(np.arange(per.size), per)
    return {"radius": float(radius), "n_pairs": int(idx.size), "rows_with_hit": int((per > 0).sum()),
            "largest_row": int(per.max()) if per.size else 0,
            "pairs": [[_name(query_names, i), _name(bank_names, c), float(v)] for i, c, v in zip(rows, idx, np.sqrt(d2))]}


def radius_line(report):
    """The ``NN-radius:`` line of ``python -m wu.fid ... --nn-radius R`` and of this module's command line."""
    return f"NN-radius: {report['radius']} pairs {report['n_pairs']} rows {report['rows_with_hit']} largest {report['largest_row']}"


# ----------------------------------------------------------------------------------------------
# per-row realism and rarity against the bank's k-NN balls
# ----------------------------------------------------------------------------------------------
BallScores = collections.namedtuple("BallScores", ["realism", "realism_index", "rarity", "rarity_index", "count", "realism_r2",
                                                   "realism_d2", "rarity_r2"])


def ball_scores(query, bank, k=3, bank_radii=None, exclude_self=False, col_splits=0):
    """Per query row, against the balls around the bank rows whose squared radii are ``bank_radii`` (``wu.prdc.knn_radii(bank, k)`` unless
    given: (nb,) float64 on the bank's device), a ``BallScores`` of CUDA tensors:

    ``realism`` (float64): the realism score of Kynkaanniemi et al. 2019, ``max_j radius_j / |q - b_j|``, formed as ``sqrt(rho)`` of the
    largest quotient ``rho = r2_j / d2_j`` (one IEEE division per pair; +inf where the row coincides with a bank row); >= 1 exactly when
    the row lies in some ball.  ``realism_index`` (int64): the maximising bank row, the smaller on equal quotients; ``realism_r2`` /
    ``realism_d2`` its two operands.
    ``rarity`` (float64): the rarity score of Han et al. 2022, the radius of the smallest ball that holds the row (``sqrt(rarity_r2)``),
    +inf for a row outside the manifold.  ``rarity_index`` (int64): that ball's bank row, the smaller on equal radii, -1 outside.
    ``count`` (int64): the number of balls that hold the row -- without ``exclude_self`` wu.prdc's ``B`` bit for bit.

    ``exclude_self``: query and bank are the same rows; row i's own ball is left out.  One walk of the tiles ``topk`` walks
    (wu_nn_ball_scores, csrc/nn_radius.hip); nothing is synchronised when the radii are given."""
    who = "ball_scores"
    _check_k(k, col_splits, who)
    q, b = _pair(query, bank, "exclude_self" if exclude_self else None, who)
    (nq, d), nb = q.shape, b.shape[0]
    if exclude_self and nb < 2:
        raise ValueError(f"{who}: the bank has n = {nb} rows, exclude_self needs at least 2")
    if bank_radii is None:
        from .prdc import knn_radii
        bank_radii = knn_radii(bank, k)
    r2 = bank_radii
    if not torch.is_tensor(r2) or r2.dtype != torch.float64 or r2.device != b.device or r2.shape != (nb,) or not r2.is_contiguous():
        raise ValueError(f"{who}: bank_radii must be a contiguous ({nb},) float64 tensor on the bank's device (wu.prdc.knn_radii)")
    lib = _lib.load()
    dev = q.device
    col_splits = int(col_splits)
    with torch.cuda.device(dev):
        nbytes = lib.wu_nn_ball_workspace_bytes(nq, nb, col_splits)
        if nbytes == 0:
            raise ValueError(f"{who}: nq = {nq} / nb = {nb} / col_splits = {col_splits} out of the library's range")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        count = torch.empty(nq, dtype=torch.int32, device=dev)
        rar_r2, rl_r2, rl_d2 = (torch.empty(nq, dtype=torch.float64, device=dev) for _ in range(3))
        rar_i, rl_i = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(2))
        _lib.call("wu_nn_ball_scores", q.data_ptr(), q.stride(0), nq, b.data_ptr(), b.stride(0), nb, d, r2.data_ptr(),
                  0 if exclude_self else -1, col_splits, ws.data_ptr(), ws.numel(), count.data_ptr(), rar_r2.data_ptr(), rar_i.data_ptr(),
                  rl_r2.data_ptr(), rl_d2.data_ptr(), rl_i.data_ptr(), stream_ptr())
        rho = torch.where(rl_d2 == 0, torch.full_like(rl_r2, float("inf")), rl_r2 / rl_d2)
        return BallScores(torch.sqrt(rho), rl_i.long(), torch.sqrt(rar_r2), rar_i.long(), count.long(), rl_r2, rl_d2, rar_r2)


def score_report(scores, m=10, k=None, query_names=None, bank_names=None):
    """A plain dict (JSON-serialisable) on a ``BallScores`` (tensors or arrays): ``n_query``, ``k`` (when given), ``realism_quantiles``
    over the finite realism scores and ``n_infinite_realism`` beside them, ``share_realism_below_1`` (the rows in no ball by the realism
    rule), ``share_in_no_ball`` (by the count; the same number), ``rarity_quantiles`` over the rows inside the manifold (QUANTILES, numpy's
    linear interpolation; empty without such rows), ``lowest_realism`` -- the m least realistic rows as ``[query, realism, bank]``, lowest
    first, ties by query index -- and ``highest_rarity`` -- the m rarest rows inside the manifold as ``[query, rarity, bank]``, highest
    first.  Names stand in place of indices where names are given.  Pure host code."""
    realism, rl_i = _host(scores.realism, np.float64), _host(scores.realism_index, np.int64)
    rarity, rar_i, count = _host(scores.rarity, np.float64), _host(scores.rarity_index, np.int64), _host(scores.count, np.int64)
    n = realism.size
    if not (rl_i.shape == rarity.shape == rar_i.shape == count.shape == realism.shape == (n,)):
        raise ValueError("score_report: the scores must be vectors of one length")
    m = max(0, int(m))

    def quantiles(v):
        return {name: float(np.quantile(v, p)) for name, p in QUANTILES} if v.size else {}

    rep = {"n_query": int(n)}
    if k is not None:
        rep["k"] = int(k)
    finite, inside = np.isfinite(realism), np.isfinite(rarity)
    rep["realism_quantiles"] = quantiles(realism[finite])
    rep["n_infinite_realism"] = int(n - finite.sum())
    rep["share_realism_below_1"] = int((realism < 1).sum()) / n if n else 0.0
    rep["share_in_no_ball"] = int((count == 0).sum()) / n if n else 0.0
    rep["rarity_quantiles"] = quantiles(rarity[inside])
    low = np.lexsort((np.arange(n), realism))[:m]
    rep["lowest_realism"] = [[_name(query_names, i), float(realism[i]), _name(bank_names, rl_i[i])] for i in low]
    rows = np.flatnonzero(inside)
    high = rows[np.lexsort((rows, -rarity[rows]))][:m]
    rep["highest_rarity"] = [[_name(query_names, i), float(rarity[i]), _name(bank_names, rar_i[i])] for i in high]
    return rep


def realism_line(report):
    """The ``Realism:`` line of ``python -m wu.fid ... --realism`` and of this module's command line."""
    q = report["realism_quantiles"]
    line = "Realism:" + (f" k {report['k']}" if "k" in report else "")
    return line + f" median {q.get('median')} below-1 {report['share_realism_below_1']} no-ball {report['share_in_no_ball']}"


# ----------------------------------------------------------------------------------------------
# the memorisation figure
# ----------------------------------------------------------------------------------------------
def figure_rows(dist2, rows):
    """The query rows the figure shows: the ``rows`` with the smallest nearest distance, closest first (ties by query index)."""
    near = _host(dist2, np.float64)[:, 0]
    order = np.lexsort((np.arange(near.size), near))
    return [int(i) for i in order[:max(0, int(rows))]]


def _read_cell(path, cell):
    """Not wu.files.read_rgb: the resize is Pillow's, on the Image, before it becomes an array."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        if im.size != (cell, cell):
            im = im.resize((cell, cell), Image.BILINEAR)
        return np.asarray(im, dtype=np.uint8)


def figure_cells(query_files, bank_files, index, rows, cell):
    """(len(rows) * (k + 1), 3, cell, cell) float32 in [0, 1] on the host: per chosen query row the query image and its k neighbours,
    re-read from the files by index and resized on the host (at most rows x (k + 1) small images: not the hot path)."""
    idx = _host(index, np.int64)
    cells = []
    for i in rows:
        cells.append(_read_cell(query_files[i], cell))
        cells.extend(_read_cell(bank_files[j], cell) for j in idx[i])
    return torch.from_numpy(np.stack(cells)).permute(0, 3, 1, 2).float().div_(255.0)


def save_figure(path, query_files, bank_files, dist2, index, rows=16, cell=128, device="cuda"):
    """Writes the figure: one row per chosen query (``figure_rows``), the query in column 0 and its neighbours, nearest first, in columns
    1..k, composed by ``wu.grid.make_grid``'s kernels and written through ``wu.infer_driver.save_grid``.  Returns the chosen rows."""
    from .infer_driver import save_grid
    chosen = figure_rows(dist2, rows)
    if not chosen:
        raise ValueError("save_figure: no rows to show")
    k = _host(index, np.int64).shape[1]
    save_grid(figure_cells(query_files, bank_files, index, chosen, cell).to(device), path, nrow=k + 1, padding=2, pad_value=1.0)
    return chosen


def save_realism_figure(path, query_files, bank_files, scores, rows=16, cell=128, device="cuda"):
    """Writes the figure of the least realistic queries: one row per query, lowest realism first (ties by query index), the query in
    column 0 and the bank image of its largest radius / distance quotient in column 1, through ``save_figure``'s grid code.  Returns the
    chosen rows."""
    from .infer_driver import save_grid
    realism = _host(scores.realism, np.float64)
    chosen = [int(i) for i in np.lexsort((np.arange(realism.size), realism))[:max(0, int(rows))]]
    if not chosen:
        raise ValueError("save_realism_figure: no rows to show")
    index = _host(scores.realism_index, np.int64)[:, None]
    save_grid(figure_cells(query_files, bank_files, index, chosen, cell).to(device), path, nrow=2, padding=2, pad_value=1.0)
    return chosen


def main(argv=None):
    from . import fid
    from .files import image_files
    from .inception import InceptionV3
    ap = argparse.ArgumentParser(prog="python -m wu.retrieval", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                 description="Nearest bank images of every query image on InceptionV3 features: the memorisation figure, "
                                             "the leakage check, near-duplicates inside one directory (--self)")
    ap.add_argument("query", help="directory of query images (or a .npz holding 'features'; then no figure)")
    ap.add_argument("bank", nargs="?", help="directory of bank images (or a .npz holding 'features'); not given with --self")
    ap.add_argument("--weights", required=True, help="pytorch-fid FID Inception weights (pt_inception-2015-12-05-*.pth)")
    ap.add_argument("--k", type=int, default=8, help="neighbours per query, 1..16; a row with more than k copies hides the rest")
    ap.add_argument("--self", dest="self_", action="store_true", help="query the one directory against itself, every image's own row skipped")
    ap.add_argument("--threshold", type=float, default=None, help="also list the nearest pairs closer than this distance")
    ap.add_argument("--rows", type=int, default=16, help="figure: the queries with the smallest nearest distance, one per row")
    ap.add_argument("--cell", type=int, default=128, help="figure: side of a cell in pixels")
    ap.add_argument("--figure", default=None, help="write the figure here (.png / .jpg)")
    ap.add_argument("--radius", type=float, default=None, metavar="R",
                    help="also find EVERY bank image within the distance R of a query image (radius_join) and print one NN-radius: line; "
                         "with --self the duplicate groups, however many copies a group holds")
    ap.add_argument("--groups", default=None, metavar="OUT.json", help="with --self --radius: write the duplicate groups (lists of file names)")
    ap.add_argument("--keep", default=None, metavar="OUT.txt",
                    help="with --radius: write the query files to keep, one per line -- with --self the files that are not a later member of "
                         "a duplicate group (the first file of each group stays), otherwise the query files with no bank image inside R")
    ap.add_argument("--realism-worst", type=int, default=0, metavar="M",
                    help="with --figure: show instead the M least realistic queries (ball_scores, --realism-k) beside their maximising bank image")
    ap.add_argument("--realism-k", type=int, default=3, help="with --realism-worst: the k of the bank's k-NN radii")
    ap.add_argument("--report", default=None, help="write nearest_report's dict here as JSON")
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--dims", type=int, default=2048, choices=list(InceptionV3.BLOCK_INDEX_BY_DIM))
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args(argv)
    if args.self_ and args.bank is not None and args.bank != args.query:
        ap.error("--self takes one directory")
    if not args.self_ and args.bank is None:
        ap.error("a bank directory, or --self")
    paths = [args.query] if args.self_ else [args.query, args.bank]
    if args.figure and any(p.endswith(".npz") for p in paths):
        ap.error("--figure needs image directories")
    if (args.groups or args.keep) and args.radius is None:
        ap.error("--groups and --keep need --radius")
    if args.groups and not args.self_:
        ap.error("--groups needs --self")
    if args.realism_worst and not args.figure:
        ap.error("--realism-worst needs --figure")
    _, banks = fid._pass_over_paths(paths, args.weights, args.batch_size, args.dims, args.precision, fid=False, rows=True)
    q, b = banks[0], banks[-1]
    files = [None if p.endswith(".npz") else image_files(p) for p in paths]
    qf, bf = files[0], files[-1]
    dist2, index = topk(q, b, args.k, exclude_self=args.self_)
    rep = report_from_topk(dist2, index, args.threshold, args.self_, None if qf is None else [f.name for f in qf],
                           None if bf is None else [f.name for f in bf], n_bank=b.n)
    print(nn_line(rep))
    if args.report:
        with open(args.report, "w") as fh:
            json.dump(rep, fh)
    if args.radius is not None:
        qn = [str(i) for i in range(q.n)] if qf is None else [f.name for f in qf]
        join = radius_join(q, b, args.radius * args.radius, unique_pairs=args.self_)
        print(radius_line(radius_report(*join, args.radius)))
        if args.self_:
            _, groups = groups_from_pairs(q.n, join[0], join[1])
            dropped = {i for g in groups for i in g[1:]}
            if args.groups:
                with open(args.groups, "w") as fh:
                    json.dump([[qn[i] for i in g] for g in groups], fh)
        else:
            dropped = set(np.flatnonzero(np.diff(_host(join[0], np.int64)) > 0).tolist())
        if args.keep:
            with open(args.keep, "w") as fh:
                fh.writelines(qn[i] + "\n" for i in range(q.n) if i not in dropped)
    if args.figure and args.realism_worst:
        scores = ball_scores(q, b, k=args.realism_k, exclude_self=args.self_)
        save_realism_figure(args.figure, qf, bf, scores, args.realism_worst, args.cell, device=q.features.device)
    elif args.figure:
        save_figure(args.figure, qf, bf, dist2, index, args.rows, args.cell, device=q.features.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
