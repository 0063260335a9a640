"""Grid composition benchmark: wu.grid (csrc/grid.hip) against the two ways to get the same pictures without it, on one MI355X.

    python scratch/bench_grid.py [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o grid -- python scratch/bench_grid.py --mode device      # kernel rows, run of its own

Workloads: the demo table of demo.py:67-82 for B=16, nc=5, 256^2, T=8 frames in one call, and the evaluation summary of
t_cls_train.py:361-378 for B=16, 224^2.  Each is timed against
  * torch ops on the device: tests/_grid_ref.py's functions (the literal make_grid loop) given CUDA tensors;
  * the reference's own route: .cpu() of the sources, then the same loop on the host.
Neither baseline is code under test; all three produce the same bits (checked outside the timing).
Method: warm-up, then `--runs` runs per path of at least `--min-seconds` each, the paths alternating; a run is timed with device events
around whole calls and ends in a synchronise; median (min .. max) per call.  Launches per call: wu_prof_* for the kernels, the CUDA
kernel events of torch.profiler for the torch-op composition.  Bytes: what the algorithm moves, from the shapes -- every source sample
read twice (ranges, compose), the output written twice (fill, cells).  Results go to profiles/grid_bench.md by hand, with the command line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12          # bytes / s, MI355X specification


def timed(fn, runs, min_seconds, device_events=True):
    """[seconds per call] over `runs` runs of whole calls lasting at least min_seconds each."""
    out = []
    for _ in range(runs):
        n, t0 = 0, time.perf_counter()
        if device_events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        while True:
            fn()
            n += 1
            if n % 4 == 0 or not device_events:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= min_seconds:
                    break
        if device_events:
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3 / n)
        else:
            out.append((time.perf_counter() - t0) / n)
    return out


def spread(v, unit=1e3):
    return f"{statistics.median(v) * unit:.3f} ({min(v) * unit:.3f} .. {max(v) * unit:.3f})"


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "device"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _grid_ref as R
    from wu import _lib, grid
    from wu import infer_driver as D
    from wu.png_enc import GPUPngEncoder

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"cmd": " ".join(sys.argv), "gpu": torch.cuda.get_device_name(0), "runs": a.runs, "min_seconds": a.min_seconds}

    T, nc, B, S = 8, 5, 16, 256
    batch = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    results = torch.tanh(torch.randn(T, nc, B, 3, S, S, generator=g)).to(dev)
    Bs, Ss = 16, 224
    images = (torch.rand(Bs, 3, Ss, Ss, generator=g) * 2 - 1).to(dev)
    refs = (torch.rand(Bs, 3, Ss, Ss, generator=g) * 2 - 1).to(dev)
    fakes = torch.tanh(torch.randn(Bs, Bs, 3, Ss, Ss, generator=g)).to(dev)

    def bytes_moved(plan, out_elem):
        f, hg, wg = plan.shape
        src = sum(3 * c.h * c.w * 4 for c in plan.cells if c.source is not None)
        cells = sum(3 * c.h * c.w * out_elem for c in plan.cells)
        return 2 * src + f * hg * wg * 3 * out_elem + cells

    cases = {
        "demo_u8": (lambda: grid.demo_tables(batch, results), lambda: R.to_u8(R.demo_tables(batch, results)),
                    lambda: R.to_u8(R.demo_tables(batch.cpu(), results.cpu())), grid.plan_demo_tables(T, nc, B, S, S), 1),
        "summary_f32": (lambda: grid.summary_image(images, refs, fakes), lambda: R.summary_image(images, refs, fakes),
                        lambda: R.summary_image(images.cpu(), refs.cpu(), fakes.cpu()), grid.plan_summary(Bs, Ss, Ss), 4),
    }
    for name, (ours, torch_ops, cpu_route, plan, out_elem) in cases.items():
        got, want = ours(), torch_ops()
        torch.cuda.synchronize()
        same = bool(torch.equal(got, want)) and bool(torch.equal(got.cpu(), cpu_route()))
        row = {"cells": len(plan.cells), "frame": list(plan.shape), "identical_to_both_baselines": same}
        if a.mode == "device":
            for _ in range(20):
                ours()
            torch.cuda.synchronize()
            res[name] = row
            continue
        _lib.prof_begin([_lib.FAM_GRID], 16)
        ours()
        q = _lib.prof_query(_lib.FAM_GRID)
        _lib.prof_end()
        row["launches"] = q["launches"]
        row["kernel_ms_one_call_events"] = round(q["ms"], 4)
        row["torch_op_launches"] = kernel_launches(torch_ops)
        for _ in range(3):
            ours(), torch_ops()
        torch.cuda.synchronize()
        t_ours, t_torch = [], []
        for r in range(a.runs):                                            # alternate the two device paths
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (t_ours if which == 0 else t_torch).extend(timed(ours if which == 0 else torch_ops, 1, a.min_seconds))
        t_cpu = timed(cpu_route, 2, 0.0, device_events=False)
        by = bytes_moved(plan, out_elem)
        row.update({"call_ms": spread(t_ours), "torch_ops_ms": spread(t_torch), "cpu_route_ms": spread(t_cpu),
                    "bytes_moved": by, "hbm_share_of_8TBps_over_call_time": round(by / statistics.median(t_ours) / HBM_PEAK, 4),
                    "speedup_vs_torch_ops": round(statistics.median(t_torch) / statistics.median(t_ours), 2),
                    "speedup_vs_cpu_route": round(statistics.median(t_cpu) / statistics.median(t_ours), 1)})
        res[name] = row
        print(name, json.dumps(row), flush=True)

    if a.mode == "all":                                                      # compose + encode + files on disk, the T demo frames
        enc = GPUPngEncoder(dev)
        with tempfile.TemporaryDirectory() as tmp:
            for ext, kw in ((".jpg", {}), (".png", {"png_encoder": enc})):
                def e2e(ext=ext, kw=kw):
                    D.save_demo(grid.demo_tables(batch, results), os.path.join(tmp, ext[1:]), ext=ext, **kw)
                e2e()
                res["demo_T8_compose_encode_write" + ext] = {"wall_ms": spread(timed(e2e, a.runs, a.min_seconds, device_events=False))}
                print(ext, res["demo_T8_compose_encode_write" + ext], flush=True)
        enc.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
