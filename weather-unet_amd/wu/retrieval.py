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
entry is a real neighbour.  A top-k search finds a duplicate unless the row has more than k copies; all pairs under a radius are not
emitted.

The distance matrix is never stored (wu_nn_topk, csrc/nn_topk.hip: 64 x 64 tiles on the fp64 matrix cores, the tile of csrc/gram_f64.h
that the KID and PRDC share, consumed by the epilogue).  There is no host fallback."""
import argparse
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
# the memorisation figure
# ----------------------------------------------------------------------------------------------
def figure_rows(dist2, rows):
    """The query rows the figure shows: the ``rows`` with the smallest nearest distance, closest first (ties by query index)."""
    near = _host(dist2, np.float64)[:, 0]
    order = np.lexsort((np.arange(near.size), near))
    return [int(i) for i in order[:max(0, int(rows))]]


def _read_cell(path, cell):
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


def main(argv=None):
    from . import fid
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
    _, banks = fid._pass_over_paths(paths, args.weights, args.batch_size, args.dims, args.precision, False, False, False, fid=False, rows=True)
    q, b = banks[0], banks[-1]
    files = [None if p.endswith(".npz") else fid.image_files(p) for p in paths]
    qf, bf = files[0], files[-1]
    dist2, index = topk(q, b, args.k, exclude_self=args.self_)
    rep = report_from_topk(dist2, index, args.threshold, args.self_, None if qf is None else [f.name for f in qf],
                           None if bf is None else [f.name for f in bf], n_bank=b.n)
    print(nn_line(rep))
    if args.report:
        with open(args.report, "w") as fh:
            json.dump(rep, fh)
    if args.figure:
        save_figure(args.figure, qf, bf, dist2, index, args.rows, args.cell, device=q.features.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
