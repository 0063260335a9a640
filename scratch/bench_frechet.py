"""Time of the rank-aware Frechet distance on feature rows (wu.frechet.frechet_distance: csrc/frechet.hip) against the two things a user
could run instead on the same rows:

  host      the path `python -m wu.fid` takes today: FIDStatistics.update_features in batches of 50 + finalize() for both sets (the D x D
            accumulators come to the host) and calculate_frechet_distance (scipy's sqrtm of the 2048 x 2048 product, on this host's CPUs);
  svdvals   torch.linalg.svdvals of the SAME centred matrix on the same GPU, in place of the Jacobi sweeps (the other stages are shared).

    python scratch/bench_frechet.py [--steps 3] [--warmup 1] [--shape 500x500 2048x2048 4096x4096 500x50000] [--no-host]

D = 2048.  Rows: x = rand, y = |x[src] + sigma randn| with sigma log-uniform in [0.05, 0.6], generated on the device from a seed.  Every
timed call is a host clock around work that ends in a device synchronise (frechet_distance reads the rotation counter once per sweep, so it
cannot be bracketed by device events alone); rows and svdvals alternate call by call; the host path, seconds long, runs once per shape.
Launches are counted from the shapes: 5 (Gram and centring) + 2 x 3 (moments) + sweeps x N Jacobi steps + 2 (finish), N = 2 ceil(ns / 2) - 1.
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

D = 2048


def make_rows(n1, n2, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.rand(n1, D, device=dev, generator=g)
    src = torch.randint(0, n1, (n2,), device=dev, generator=g)
    sigma = torch.exp(torch.rand(n2, device=dev, generator=g) * (np.log(0.6) - np.log(0.05)) + np.log(0.05))
    y = torch.empty(n2, D, device=dev)
    for lo in range(0, n2, 16384):
        hi = min(n2, lo + 16384)
        y[lo:hi] = (x[src[lo:hi]] + sigma[lo:hi, None] * torch.randn(hi - lo, D, device=dev, generator=g)).abs_()
    return x, y


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shape", nargs="+", default=["500x500", "2048x2048", "4096x4096", "500x50000"])
    ap.add_argument("--no-host", action="store_true", help="skip the host path (sqrtm of a 2048 x 2048 product takes tens of seconds)")
    a = ap.parse_args()
    from wu import _lib, fid, frechet
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for shape in a.shape:
        n1, n2 = (int(v) for v in shape.split("x"))
        torch.cuda.empty_cache()
        x, y = make_rows(n1, n2, dev, seed=n1 + n2)
        ns = min(n1, n2)
        n_steps = 2 * ((ns + 1) // 2) - 1

        def front():
            v, ws = frechet.centred_cross_gram(x, y)
            (mu1, _, s1), (mu2, _, s2) = frechet.moments(x), frechet.moments(y)
            return v, ws, mu1, s1, mu2, s2

        def with_svdvals():
            v, _ws, mu1, s1, mu2, s2 = front()
            total = torch.linalg.svdvals(v.contiguous()).sum().item()
            d = (mu1 - mu2).cpu().numpy()
            return ((float(np.dot(d, d)) + s1.item() / (n1 - 1)) + s2.item() / (n2 - 1)) - 2.0 * total / np.sqrt((n1 - 1.0) * (n2 - 1.0))

        rows_ms, svd_ms, front_ms, r, svd_fid, svd_err = [], [], [], None, None, None
        for i in range(a.warmup + a.steps):
            t, r = timed(lambda: frechet.frechet_distance(x, y))
            tf, _ = timed(front)
            if i >= a.warmup:
                rows_ms.append(t)
                front_ms.append(tf)
            if svd_err is None:
                try:
                    t, svd_fid = timed(with_svdvals)
                    if i >= a.warmup:
                        svd_ms.append(t)
                except RuntimeError as e:                # reported, not hidden
                    svd_err = str(e).splitlines()[0]
                    torch.cuda.empty_cache()
        res = {"n1": n1, "n2": n2, "D": D, "steps": a.steps, "warmup": a.warmup,
               "rows_ms_median": round(float(np.median(rows_ms)), 2), "rows_ms_all": [round(t, 2) for t in rows_ms],
               "front_ms_median": round(float(np.median(front_ms)), 2),
               "sweeps": r.sweeps, "rotations": r.rotations, "launches": 5 + 6 + r.sweeps * n_steps + 2,
               "workspace_bytes": int(lib.wu_fd_workspace_bytes(n1, n2, D)), "rows_fid": r.fid,
               "svdvals_ms_median": round(float(np.median(svd_ms)), 2) if svd_ms else None, "svdvals_ms_all": [round(t, 2) for t in svd_ms],
               "svdvals_fid": svd_fid, "svdvals_error": svd_err,
               "abs_diff_rows_svdvals": None if svd_fid is None else abs(r.fid - svd_fid), "device": torch.cuda.get_device_name(0)}
        if not a.no_host:
            def host():
                out = []
                for rows in (x, y):
                    st = fid.FIDStatistics(None)
                    for lo in range(0, rows.shape[0], 50):        # python -m wu.fid's default --batch-size
                        st.update_features(rows[lo:lo + 50])
                    out.append(st.finalize())
                return fid.calculate_frechet_distance(*out[0], *out[1])
            t, host_fid = timed(host)
            res.update({"host_ms": round(t, 1), "host_fid": host_fid, "abs_diff_rows_host": abs(r.fid - host_fid),
                        "abs_diff_svdvals_host": None if svd_fid is None else abs(svd_fid - host_fid),
                        "host_threads": os.environ.get("OMP_NUM_THREADS")})
        print(json.dumps(res), flush=True)
        del x, y, r


if __name__ == "__main__":
    main()
