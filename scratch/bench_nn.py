"""Device time of top-k nearest-neighbour retrieval on the fused path (wu.retrieval.topk -> wu_nn_topk: csrc/nn_topk.hip) and of the
torch-op composition a user would write on the same GPU: torch.cdist on float64 + torch.topk(largest=False), chunked over the queries where
the distance matrix would not fit.

    python scratch/bench_nn.py [--steps 5] [--warmup 2] [--config split mid self50k self215k] [--chunk-bytes N] [--col-splits S] [--no-composition]

  split      500 x 500, the bank against itself          the 500-photograph test split
  mid        2 500 queries x 50 000 bank rows
  self50k    50 000 against itself
  self215k   215 000 against itself                       the training set: only the chunked composition can run

D = 2048, k = 8.  Rows: x = rand, queries y = |x[src] + sigma randn| with sigma log-uniform in [0.05, 0.6], generated on the device from a
seed (scratch/bench_prdc.py's).  The composition holds the bank in float64 once per call and walks the queries in chunks whose
chunk x nb float64 matrix stays within --chunk-bytes (8 GiB unless given; one chunk where the whole matrix fits); against itself it sets
the chunk's diagonal to +inf before topk.  Each timed call is bracketed by device events and followed by a device synchronise; the two
paths alternate call by call.  Peak memory is torch's max_memory_allocated over the call minus what was allocated before it (the rows
themselves are not counted).  FLOP count of the fused path: 2 D per entry in whole 64 x 64 tiles.  One JSON line per config."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

D, K = 2048, 8
CONFIGS = {"split": (500, 500, True), "mid": (2500, 50000, False), "self50k": (50000, 50000, True), "self215k": (215000, 215000, True)}


def make_rows(n, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.rand(n, D, device=dev, generator=g), g


def make_queries(x, nq, g):
    n, dev = x.shape[0], x.device
    src = torch.randint(0, n, (nq,), device=dev, generator=g)
    sigma = torch.exp(torch.rand(nq, device=dev, generator=g) * (np.log(0.6) - np.log(0.05)) + np.log(0.05))
    y = torch.empty(nq, D, device=dev)
    for lo in range(0, nq, 16384):
        hi = min(nq, lo + 16384)
        y[lo:hi] = (x[src[lo:hi]] + sigma[lo:hi, None] * torch.randn(hi - lo, D, device=dev, generator=g)).abs_()
    return y


def composition(q, b, k, own, chunk_rows):
    """(distance (nq, k), index (nq, k)): cdist gives distances, not squared ones."""
    b64 = b.double()
    dist = torch.empty(q.shape[0], k, dtype=torch.float64, device=q.device)
    index = torch.empty(q.shape[0], k, dtype=torch.int64, device=q.device)
    for r0 in range(0, q.shape[0], chunk_rows):
        r1 = min(q.shape[0], r0 + chunk_rows)
        d = torch.cdist(b64[r0:r1] if own else q[r0:r1].double(), b64)
        if own:
            rows = torch.arange(r1 - r0, device=q.device)
            d[rows, rows + r0] = float("inf")
        v, i = torch.topk(d, k, dim=1, largest=False)
        dist[r0:r1], index[r0:r1] = v, i
        del d
    return dist, index


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--chunk-bytes", type=int, default=8 << 30)
    ap.add_argument("--no-composition", action="store_true")
    ap.add_argument("--col-splits", type=int, default=0, help="forced bank column splits of the fused path (0: the library's choice)")
    a = ap.parse_args()
    from wu import _lib, retrieval
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for name in a.config:
        torch.cuda.empty_cache()
        nq, nb, own = CONFIGS[name]
        big = nq * nb > 1 << 31
        steps, warmup = (max(2, a.steps // 2), 1) if big else (a.steps, a.warmup)
        x, g = make_rows(nb, dev, seed=nb)
        q = x if own else make_queries(x, nq, g)
        chunk_rows = max(1, min(nq, a.chunk_bytes // (8 * nb)))
        fused_ms, comp_ms, fused_peak, comp_peak, comp_err, comp_out = [], [], 0, None, None, None
        for i in range(warmup + steps):
            t, peak, out = timed(lambda: retrieval.topk(q, x, K, exclude_self=own, col_splits=a.col_splits))
            if i >= warmup:
                fused_ms.append(t)
                fused_peak = max(fused_peak, peak)
            if not a.no_composition and comp_err is None:
                try:
                    t, peak, comp_out = timed(lambda: composition(q, x, K, own, chunk_rows))
                    if i >= warmup:
                        comp_ms.append(t)
                        comp_peak = max(comp_peak or 0, peak)
                except torch.OutOfMemoryError as e:
                    comp_err = "out of memory: " + str(e).splitlines()[0]
                    torch.cuda.empty_cache()
        ms = float(np.median(fused_ms))
        tq, tb = (nq + 63) // 64, (nb + 63) // 64
        res = {"config": name, "nq": nq, "nb": nb, "D": D, "k": K, "exclude_self": own, "steps": steps, "warmup": warmup,
               "fused_ms_median": round(ms, 3), "fused_ms_all": [round(t, 3) for t in fused_ms],
               "col_splits": a.col_splits,
               "fused_workspace_bytes": int(lib.wu_nn_workspace_bytes(nq, nb, K, a.col_splits)), "fused_peak_bytes": int(fused_peak),
               "tflops_fp64_tiles": round(2.0 * D * 64 * 64 * tq * tb / ms / 1e9, 2), "device": torch.cuda.get_device_name(0)}
        if not a.no_composition:
            res.update({"composition_chunk_rows": chunk_rows, "composition_ms_median": round(float(np.median(comp_ms)), 3) if comp_ms else None,
                        "composition_ms_all": [round(t, 3) for t in comp_ms], "composition_peak_bytes": comp_peak, "composition_error": comp_err})
            if comp_out is not None:
                same = (out[1] == comp_out[1])
                res["index_agreement"] = round(same.float().mean().item(), 6)
                res["max_abs_distance_difference"] = float((out[0].sqrt() - comp_out[0]).abs().max().item())
        print(json.dumps(res), flush=True)
        del x, q, out, comp_out


if __name__ == "__main__":
    main()
