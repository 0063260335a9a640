"""Device time of the radius join and the ball scores on the fused path (wu.retrieval.radius_join -> wu_nn_radius_count / wu_nn_radius_fill,
wu.retrieval.ball_scores -> wu_nn_ball_scores: csrc/nn_radius.hip) against the torch-op composition a user would write on the same GPU and
against wu.retrieval.topk at k = 16 on the same rows, all from one process.

    python scratch/bench_radius.py [--steps 3] [--warmup 1] [--config split mid self50k self215k] [--chunk-bytes N] [--col-splits S] [--no-composition]

Sizes and rows are scratch/bench_nn.py's (D = 2048).  Two radii per size, estimated from the float64 distances of 4096 x 4096 sampled rows:
the 1e-5 quantile of d^2 (a dedup radius: nearly empty) and the 1 % quantile (a dense one).  The join composition holds the bank in float64
once per call and walks the queries in chunks whose chunk x nb float64 matrix stays within --chunk-bytes (8 GiB unless given):
torch.cdist, the diagonal set to +inf where the bank is joined with itself, `d <= sqrt(radius2)`, nonzero, and the gather of the
distances.  The score composition squares the same chunk matrix and takes the three reductions (membership count, the smallest radius
among the balls that hold the row, the largest r2 / d2 with its column).  Both fused paths get the bank's radii from one
wu.prdc.knn_radii call outside the timing.  One warm-up, then the paths alternate call by call; each timed call is bracketed by device
events and followed by a device synchronise; peak memory is torch's max_memory_allocated over the call minus what was allocated before it.
One JSON line per (config, measurement)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "scratch")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_nn import CONFIGS, D, make_queries, make_rows, timed  # noqa: E402

K_TOPK, K_BALL = 16, 3
QUANTILES = (("dedup", 1e-5), ("dense", 1e-2))


def sample_radii(q, b, own, g):
    """The quantiles of d^2 over 4096 x 4096 sampled rows (all rows of a smaller side); a row against itself does not count."""
    qi = torch.randperm(q.shape[0], device=q.device, generator=g)[:4096]
    bi = torch.randperm(b.shape[0], device=q.device, generator=g)[:4096]
    d = torch.cdist(q[qi].double(), b[bi].double())
    if own:
        d[qi[:, None] == bi[None, :]] = float("inf")
    d2 = (d * d).flatten()
    d2 = d2[torch.isfinite(d2)].sort().values
    return {name: float(d2[int(p * (d2.numel() - 1))].item()) for name, p in QUANTILES}


def join_composition(q, b, radius2, own, chunk_rows):
    b64 = b.double()
    r = float(np.sqrt(radius2))
    counts, cols, dist = [], [], []
    for r0 in range(0, q.shape[0], chunk_rows):
        r1 = min(q.shape[0], r0 + chunk_rows)
        d = torch.cdist(b64[r0:r1] if own else q[r0:r1].double(), b64)
        if own:
            rows = torch.arange(r1 - r0, device=q.device)
            d[rows, rows + r0] = float("inf")
        mask = d <= r
        counts.append(mask.sum(dim=1))
        cols.append(mask.nonzero()[:, 1])
        dist.append(d[mask])
        del d, mask
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=q.device), torch.cat(counts).cumsum(0)])
    return row_ptr, torch.cat(cols), torch.cat(dist)


def ball_composition(q, b, r2, own, chunk_rows):
    b64 = b.double()
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=q.device)
    out = [[] for _ in range(5)]
    for r0 in range(0, q.shape[0], chunk_rows):
        r1 = min(q.shape[0], r0 + chunk_rows)
        d2 = torch.cdist(b64[r0:r1] if own else q[r0:r1].double(), b64).square_()
        if own:
            rows = torch.arange(r1 - r0, device=q.device)
            d2[rows, rows + r0] = float("inf")
        inside = d2 <= r2[None, :]
        rar, rar_i = torch.where(inside, r2[None, :], inf).min(dim=1)
        rho, rho_i = (r2[None, :] / d2).max(dim=1)
        for o, v in zip(out, (inside.sum(dim=1), rar, rar_i, rho, rho_i)):
            o.append(v)
        del d2, inside
    return [torch.cat(o) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--chunk-bytes", type=int, default=8 << 30)
    ap.add_argument("--no-composition", action="store_true")
    ap.add_argument("--col-splits", type=int, default=0, help="forced bank column splits of the fused paths (0: the library's choice)")
    a = ap.parse_args()
    from wu import _lib, prdc, retrieval
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for name in a.config:
        torch.cuda.empty_cache()
        nq, nb, own = CONFIGS[name]
        x, g = make_rows(nb, dev, seed=nb)
        q = x if own else make_queries(x, nq, g)
        radii = sample_radii(q, x, own, g)
        r2 = prdc.knn_radii(x, K_BALL)
        chunk_rows = max(1, min(nq, a.chunk_bytes // (8 * nb)))
        paths = {f"join_{kind}": (lambda r=r: retrieval.radius_join(q, x, r, exclude_self=own, col_splits=a.col_splits)) for kind, r in radii.items()}
        paths["topk16"] = lambda: retrieval.topk(q, x, K_TOPK, exclude_self=own)
        paths["ball"] = lambda: retrieval.ball_scores(q, x, K_BALL, bank_radii=r2, exclude_self=own, col_splits=a.col_splits)
        if not a.no_composition:
            for kind, r in radii.items():
                paths[f"join_{kind}_composition"] = lambda r=r: join_composition(q, x, r, own, chunk_rows)
            paths["ball_composition"] = lambda: ball_composition(q, x, r2, own, chunk_rows)
        order = sorted(paths, key=lambda n: (n.split("_")[0], n))          # a fused path right before its composition
        ms, peak, outs, errs = {n: [] for n in paths}, {n: 0 for n in paths}, {}, {}
        for i in range(a.warmup + a.steps):
            for n in order:
                if n in errs:
                    continue
                try:
                    t, p, out = timed(paths[n])
                except torch.OutOfMemoryError as e:
                    errs[n] = "out of memory: " + str(e).splitlines()[0]
                    torch.cuda.empty_cache()
                    continue
                if i >= a.warmup:
                    ms[n].append(t)
                    peak[n] = max(peak[n], p)
                outs[n] = [int(out[0][-1].item())] if n.startswith("join") else None
                if n == "ball":
                    outs[n] = [int((out.count == 0).sum().item())]
                if n == "ball_composition":
                    outs[n] = [int((out[0] == 0).sum().item())]
                del out
        tq, tb = (nq + 63) // 64, (nb + 63) // 64
        for n in order:
            res = {"config": name, "path": n, "nq": nq, "nb": nb, "D": D, "exclude_self": own, "steps": a.steps, "warmup": a.warmup,
                   "ms_median": round(float(np.median(ms[n])), 3) if ms[n] else None, "ms_all": [round(t, 3) for t in ms[n]],
                   "peak_bytes": int(peak[n]), "error": errs.get(n), "device": torch.cuda.get_device_name(0)}
            if n.startswith("join"):
                kind = n.split("_")[1]
                res.update({"radius2": radii[kind], "pairs": outs.get(n, [None])[0]})
            if n.startswith("ball"):
                res.update({"k": K_BALL, "rows_in_no_ball": outs.get(n, [None])[0]})
            if n.startswith("join") and not n.endswith("composition"):
                res.update({"col_splits": a.col_splits, "workspace_bytes": int(lib.wu_nn_radius_workspace_bytes(nq, nb, a.col_splits))})
            if n == "ball":
                res.update({"col_splits": a.col_splits, "workspace_bytes": int(lib.wu_nn_ball_workspace_bytes(nq, nb, a.col_splits))})
            if n.endswith("composition"):
                res["chunk_rows"] = chunk_rows
            elif ms[n]:
                # one full walk of the tiles over the whole call's time: the join walks them up to twice
                res["tflops_fp64_one_walk"] = round(2.0 * D * 64 * 64 * tq * tb / res["ms_median"] / 1e9, 2)
            print(json.dumps(res), flush=True)
        del x, q, r2, paths


if __name__ == "__main__":
    main()
