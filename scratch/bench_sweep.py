"""Shared-encoder condition sweep against the per-row / repeated-batch paths it replaces, same process, same GPU, same inputs.

    python scratch/bench_sweep.py [--pairs 5] [--min-seconds 0.3] [--train] [--out FILE.json]

Cases (Conditional_UNet(5, bf16); eval mode unless --train, which leaves Dropout(0.3) active as the reference's scripts do):

  class512_eager    class_sweep at 512^2, B=16: 5 eager forwards                      vs  class_sweep(shared_encoder=True)
  class512_graph    the same through hipGraphs: 5 GraphedUNet replays                 vs  one GraphedSweep replay
                    (default: one row per decoder chunk, bit-identical to the loop; *_1chunk: all 5 rows in one decoder pass of 80 images)
  rows224           one 224^2 image under 64 rows: transfer_rows on the 64-fold repeat vs  image_rows
  eval224           WeatherTransferStep.evaluation at 224^2, B=16 (16 x 16 pairs)     vs  evaluation(shared_encoder=True)

The baseline of every case is the code path the parent commit has (the flag off); its kernels are unchanged.  Per case: outputs compared once
(eval mode: bit-identical), two warm-up calls per path, then `--pairs` pairs of runs of at least `--min-seconds` each, the two paths
alternating and the order swapped every pair.  Reported: ms per call, median (min .. max) over the runs; the ratio sweep / baseline of every
pair, its median and range, and whether every pair favours the sweep -- next to the FLOP ratio it should approach (encoder 26.8 of 84.8
GFLOP per 256^2 image: (26.8 + R * 58.0) / (R * 84.8)).  Results go to profiles/sweep_bench.md by hand, with the command line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "weather-unet_amd"))


def flop_ratio(rows):
    return (26.8 + rows * 58.0) / (rows * 84.8)


def timed(fn, min_seconds):
    """ms per call over a run of at least `min_seconds` (whole calls; the device is drained before and after)."""
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 2 == 0 or calls == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= min_seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_case(name, rows, baseline, sweep, expect_identical, args):
    out_b, out_s = baseline(), sweep()
    assert out_b.shape == out_s.shape
    identical, max_diff = bool(torch.equal(out_b, out_s)), (out_b - out_s).abs().max().item()
    if expect_identical and not identical:
        raise SystemExit(f"{name}: outputs differ (max abs {max_diff:.3e}) where they must be bit-identical")
    del out_b, out_s
    for _ in range(2):
        baseline()
        sweep()
    tb, ts = [], []
    for k in range(args.pairs):
        order = (("b", baseline), ("s", sweep)) if k % 2 == 0 else (("s", sweep), ("b", baseline))
        for tag, fn in order:
            (tb if tag == "b" else ts).append(timed(fn, args.min_seconds))
    ratios = [s / b for s, b in zip(ts, tb)]
    res = {"case": name, "rows": rows, "identical_outputs": identical, "max_abs_diff": max_diff, "baseline_ms": spread(tb), "sweep_ms": spread(ts),
           "ratio": spread(ratios), "pair_ratios": [round(r, 4) for r in ratios], "every_pair_favours_sweep": all(r < 1 for r in ratios),
           "flop_ratio": round(flop_ratio(rows), 4)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--train", action="store_true", help="leave the generator's dropout active (outputs then differ by design)")
    ap.add_argument("--cases", default="class512_eager,class512_graph,rows224,eval224")
    ap.add_argument("--out")
    args = ap.parse_args()
    import cunet
    from wu import infer_driver as D
    from wu.graph_infer import GraphedSweep, GraphedUNet
    from wu.train_step import WeatherTransferStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    nc = 5
    net = cunet.Conditional_UNet(nc, precision="bf16").to(dev).train(args.train)
    g = torch.Generator().manual_seed(0)
    same = not args.train            # eval mode: the outputs must be bit-identical (the *_1chunk cases excepted: another AdaIN split count)
    results = []
    cases = args.cases.split(",")
    with torch.no_grad():
        if "class512_eager" in cases or "class512_graph" in cases:
            x = (torch.rand((16, 3, 512, 512), generator=g) * 2 - 1).to(dev)
            # default: one row per decoder chunk (bit-identical to the loop); "_1chunk": all 80 virtual images in one decoder pass
            if "class512_eager" in cases:
                results.append(run_case("class512_eager", nc, lambda: D.class_sweep(net, x), lambda: D.class_sweep(net, x, shared_encoder=True),
                                        same, args))
                results.append(run_case("class512_eager_1chunk", nc, lambda: D.class_sweep(net, x),
                                        lambda: D.class_sweep(net, x, shared_encoder=True, max_images=80), False, args))
            if "class512_graph" in cases:
                gu = GraphedUNet(net, 16, 512)
                for tag, mi in (("class512_graph", 16), ("class512_graph_1chunk", 80)):
                    gs = GraphedSweep(net, 16, 512, nc, max_images=mi)
                    results.append(run_case(tag, nc, lambda: D.class_sweep(net, x, graphed=gu),
                                            lambda: D.class_sweep(net, x, graphed=gs, shared_encoder=True),
                                            same and mi == 16, args))
                    del gs
                del gu
            del x
            torch.cuda.empty_cache()
        if "rows224" in cases:
            img = (torch.rand((1, 3, 224, 224), generator=g) * 2 - 1).to(dev)
            sig = torch.randn((64, nc), generator=g).to(dev)
            rep = img.repeat(64, 1, 1, 1)
            results.append(run_case("rows224", 64, lambda: D.transfer_rows(net, rep, sig), lambda: D.image_rows(net, img, sig), same, args))
        if "eval224" in cases:
            step = WeatherTransferStep(num_classes=nc, mode="est", device=dev)
            step.inference.train(args.train)
            step.discriminator.eval()
            x = (torch.rand((16, 3, 224, 224), generator=g) * 2 - 1).to(dev)
            labels, ref = torch.randn((16, nc), generator=g).to(dev), torch.randn((16, nc), generator=g).to(dev)
            results.append(run_case("eval224", 16, lambda: step.evaluation(x, labels, ref)[1],
                                    lambda: step.evaluation(x, labels, ref, shared_encoder=True)[1], same, args))
    print("| case | baseline ms | sweep ms | ratio sweep / baseline | FLOP ratio | every pair favours the sweep |")
    print("|---|---|---|---|---|---|")
    for r in results:
        f = lambda d, n=2: f"{d['median']:.{n}f} ({d['min']:.{n}f} .. {d['max']:.{n}f})"       # noqa: E731
        print(f"| {r['case']} | {f(r['baseline_ms'])} | {f(r['sweep_ms'])} | {f(r['ratio'], 3)} | {r['flop_ratio']:.3f} | "
              f"{'yes' if r['every_pair_favours_sweep'] else 'NO'} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "train": args.train, "pairs": args.pairs, "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
