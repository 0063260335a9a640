"""Device time of improved precision / recall and density / coverage on the fused path (wu_knn_radii on each bank, then wu_prdc_counts:
csrc/prdc.hip) and of the torch-op composition a user would write on the same GPU: torch.cdist on float64, kthvalue, comparisons, with the
three n x n float64 matrices held as the prdc package holds them.

    python scratch/bench_prdc.py [--steps 5] [--warmup 2] [--config small fit large] [--fit-n N] [--large-n N]

  small   n1 = n2 = 500, D = 2048        the 500-photograph test split
  fit     n1 = n2 = the largest n (a multiple of 1000) whose composition fits: 4 float64 n x n matrices (the three it holds and the copy
          kthvalue sorts) plus 2 bool ones within 80 % of the device's free memory, unless --fit-n gives it; an out-of-memory error of
          the composition is reported, not hidden
  large   n1 = n2 = 200 000 (--large-n)  dataset scale: the fused path alone (time and workspace bytes)

Rows: x = rand, y = |x[src] + sigma randn| with sigma log-uniform in [0.05, 0.6], generated on the device from a seed.  k = 5.
FLOP count: 2 D per entry of the three distance matrices the launches compute, in whole 64 x 64 tiles, 2 D 64^2 (T1^2 + T2^2 + T1 T2); the
dense count 2 D (n1^2 + n2^2 + n1 n2) is reported beside it.  Each timed call is bracketed by device events and followed by a device
synchronise; the two paths alternate call by call.  One JSON line per config."""
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

D, K = 2048, 5


def make_rows(n, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.rand(n, D, device=dev, generator=g)
    src = torch.randint(0, n, (n,), device=dev, generator=g)
    sigma = torch.exp(torch.rand(n, device=dev, generator=g) * (np.log(0.6) - np.log(0.05)) + np.log(0.05))
    y = torch.empty(n, D, device=dev)
    for lo in range(0, n, 16384):          # in pieces: no second n x D temporary at dataset scale
        hi = min(n, lo + 16384)
        y[lo:hi] = (x[src[lo:hi]] + sigma[lo:hi, None] * torch.randn(hi - lo, D, device=dev, generator=g)).abs_()
    return x, y


def composition(x, y, k):
    """The torch-op composition: distances (not squared), as prdc computes them."""
    x64, y64 = x.double(), y.double()
    dxx, dyy, dxy = torch.cdist(x64, x64), torch.cdist(y64, y64), torch.cdist(x64, y64)
    rx = dxx.kthvalue(k + 1, dim=1).values
    ry = dyy.kthvalue(k + 1, dim=1).values
    in_x = dxy <= rx[:, None]
    in_y = dxy <= ry[None, :]
    A, B, C = in_x.sum(dim=1), in_y.sum(dim=1), in_x.sum(dim=0)
    n1, n2 = x.shape[0], y.shape[0]
    return ((C > 0).sum().item() / n2, (B > 0).sum().item() / n1, C.sum().item() / (k * n2), (A > 0).sum().item() / n1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", nargs="+", default=["small", "fit", "large"], choices=["small", "fit", "large"])
    ap.add_argument("--fit-n", type=int, default=0)
    ap.add_argument("--large-n", type=int, default=200000)
    a = ap.parse_args()
    from wu import _lib, prdc
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for name in a.config:
        torch.cuda.empty_cache()
        if name == "small":
            n = 500
        elif name == "large":
            n = a.large_n
        else:
            free, _ = torch.cuda.mem_get_info()
            n = a.fit_n or int((0.8 * free / (4 * 8 + 2)) ** 0.5) // 1000 * 1000
        with_comp = name != "large"
        steps, warmup = (a.steps, a.warmup) if name == "small" else (max(2, a.steps // 2), 1)
        x, y = make_rows(n, dev, seed=n)

        def fused():
            a_, b_, c_, _, _ = prdc.manifold_counts(x, y, K)
            return a_, b_, c_

        fused_ms, comp_ms, comp_out, comp_err, comp_peak = [], [], None, None, None
        for i in range(warmup + steps):
            t, out = timed(fused)
            if i >= warmup:
                fused_ms.append(t)
            if with_comp and comp_err is None:
                try:
                    torch.cuda.reset_peak_memory_stats()
                    t, comp_out = timed(lambda: composition(x, y, K))
                    comp_peak = torch.cuda.max_memory_allocated()
                    if i >= warmup:
                        comp_ms.append(t)
                except torch.OutOfMemoryError as e:
                    comp_err = "out of memory: " + str(e).splitlines()[0]
                    torch.cuda.empty_cache()
        m = prdc.metrics_from_counts(*out, K)
        T = (n + 63) // 64
        ms = float(np.median(fused_ms))
        res = {"config": name, "n1": n, "n2": n, "D": D, "k": K, "steps": steps, "warmup": warmup,
               "fused_ms_median": round(ms, 3), "fused_ms_all": [round(t, 3) for t in fused_ms],
               "fused_workspace_bytes": int(lib.wu_prdc_workspace_bytes(n, n, K, 0)),
               "tflops_fp64_tiles": round(3 * 2.0 * D * 64 * 64 * T * T / ms / 1e9, 2),
               "tflops_fp64_dense": round(3 * 2.0 * D * n * n / ms / 1e9, 2),
               "fused_prdc": list(m), "device": torch.cuda.get_device_name(0)}
        if with_comp:
            res.update({"composition_ms_median": round(float(np.median(comp_ms)), 3) if comp_ms else None,
                        "composition_ms_all": [round(t, 3) for t in comp_ms], "composition_peak_bytes": comp_peak,
                        "composition_error": comp_err, "composition_prdc": list(comp_out) if comp_out else None})
        print(json.dumps(res), flush=True)
        del x, y, out, comp_out


if __name__ == "__main__":
    main()
