"""Device time of the Kernel Inception Distance's two launches (wu_kid_mmd: kid_gram_kernel + kid_finish_kernel) and the wall time of the
numpy restatement (tests/_kid_ref.py) on the same host -- what a user runs today.

    python scratch/bench_kid.py [--steps 5] [--warmup 2] [--numpy-subsets 4] [--config small large]

  small   n1 = n2 = 500, m = 500, S = 100, D = 2048     (the 500-photograph test split: every subset is the whole split)
  large   n1 = n2 = 10000, m = 1000, S = 100, D = 2048  (KID's customary settings)

FLOP count: 2 D per kernel-matrix entry the launch computes, in whole 64 x 64 tiles: 2 D 64^2 (T (T + 1) + T^2) per subset with
T = ceil(m / 64); the count a dense evaluation needs, 2 D (m (m - 1) + m^2), is reported beside it (the tiles compute the symmetric halves
of xx / yy once, so it can exceed the tile count).  The numpy time is measured on --numpy-subsets subsets and scaled to S.  One JSON line per config."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _kid_ref as R  # noqa: E402

CONFIGS = {"small": (500, 500, 100), "large": (10000, 1000, 100)}
D = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-subsets", type=int, default=4)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    a = ap.parse_args()
    from wu import _lib, kid
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for name in a.config:
        n, m, S = CONFIGS[name]
        rng = np.random.RandomState(0)
        x = rng.rand(n, D).astype(np.float32)
        y = (1.1 * rng.rand(n, D)).astype(np.float32)
        idx = kid.subset_indices(n, n, S, m, 2020)
        xd, yd, idd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(idx).to(dev)
        ws = torch.empty(lib.wu_kid_workspace_bytes(S, m), dtype=torch.uint8, device=dev)
        sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
        mmd2 = torch.empty(S, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def run():
            _lib.call("wu_kid_mmd", xd.data_ptr(), D, n, yd.data_ptr(), D, n, idd.data_ptr(), S, m, D, 3, 1.0 / D, 1.0, ws.data_ptr(),
                      sums.data_ptr(), mmd2.data_ptr(), stream)

        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        T = (m + 63) // 64
        flop_tiles = 2.0 * D * 64 * 64 * (T * (T + 1) + T * T) * S
        flop_useful = 2.0 * D * (m * (m - 1) + m * m) * S
        got = mmd2.cpu().numpy()
        k = min(a.numpy_subsets, S)
        t0 = time.perf_counter()
        _, ref = R.subsets(x, y, idx[:k])
        numpy_s = (time.perf_counter() - t0) * S / k
        print(json.dumps({"config": name, "n": n, "m": m, "S": S, "D": D, "steps": a.steps, "warmup": a.warmup,
                          "device_ms_median": round(ms, 3), "device_ms_all": [round(t, 3) for t in times],
                          "tflops_fp64_tiles": round(flop_tiles / ms / 1e9, 2), "tflops_fp64_useful": round(flop_useful / ms / 1e9, 2),
                          "numpy_s_scaled_to_S": round(numpy_s, 2), "numpy_subsets_timed": k, "numpy_threads": os.environ.get("OMP_NUM_THREADS"),
                          "kid_mean": float(np.mean(got)), "kid_std": float(np.std(got)),
                          "max_abs_diff_vs_numpy": float(np.abs(got[:k] - ref).max()), "bound": float(R.bound(R.subsets(x, y, idx[:1])[0], m, D)[0]),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
