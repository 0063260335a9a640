"""Device time of the fused paired-metrics call (wu.paired.pair_stats -> wu_ssim_pairs, csrc/ssim.hip, 2 * levels launches) against the torch
composition of the same numbers on the same GPU: grouped conv2d (the window as a column, then as a row) + avg_pool2d, in float64 and in
float32, the x side repeated for every row as the sweep layout makes a composition do.

    python scratch/bench_ssim.py [--steps 10] [--warmup 3] [--config sweep class u8] [--no-eval]

  sweep   R = 16, B = 16, 3 x 224 x 224, bfloat16, value range (-1, 1)   (the evaluation sweep)
  class   R = 5,  B = 16, 3 x 512 x 512, float32                         (the class sweep)
  u8      R = 1,  B = 64, 3 x 224 x 224, uint8 NHWC as a permuted view   (decoded files)

All with the 11-tap window and 5 levels (SSIM and MS-SSIM from one pass).  Per config one JSON line: median device time of the fused call and
of the two compositions (device events around one call, inputs resident), the fused call's launches and workspace bytes, the peak extra
device memory of each (torch.cuda.max_memory_allocated above the resident inputs), the torch op calls of a composition (each at least one
launch), and how far the compositions' SSIM / MS-SSIM lie from the fused fp64 values.  Unless --no-eval, a last line times
ClassTransferEval.update (5 classes, B = 16, 224 x 224, bf16 generator in eval mode, StandInEstimator as the classifier) with and without
content=ContentPreservation(): the metric's share of an evaluation step."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIGS = {"sweep": (16, 16, 224, torch.bfloat16, (-1, 1)), "class": (5, 16, 512, torch.float32, (-1, 1)), "u8": (1, 64, 224, torch.uint8, "uint8")}
K, LEVELS = 11, 5
OPS = [0]


def op(v):
    OPS[0] += 1
    return v


def composition(x, y, dtype, scale, shift, L, g):
    """(ssim (R, B), ms_ssim (R, B)) by torch ops in `dtype`; every torch call goes through op() to be counted."""
    r, b, c = y.shape[0], y.shape[1], y.shape[2]
    xm = op(op(x.to(dtype)) * scale + shift)
    ym = op(op(y.to(dtype)) * scale + shift).flatten(0, 1)
    xm = op(xm.repeat(r, 1, 1, 1))
    col = g.to(dtype).view(1, 1, -1, 1).repeat(c, 1, 1, 1)
    row = g.to(dtype).view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2

    def filt(v):
        return op(F.conv2d(op(F.conv2d(v, col, groups=c)), row, groups=c))

    vals = []
    for l in range(LEVELS):
        mux, muy = filt(xm), filt(ym)
        mxx, myy, mxy = op(mux * mux), op(muy * muy), op(mux * muy)
        sx, sy, sxy = op(filt(op(xm * xm)) - mxx), op(filt(op(ym * ym)) - myy), op(filt(op(xm * ym)) - mxy)
        cs = op(op(2 * sxy + c2) / op(op(sx + sy) + c2))
        if l == 0 or l == LEVELS - 1:
            ss = op(op(op(2 * mxy + c1) / op(op(mxx + myy) + c1)) * cs)
            if l == 0:
                ssim = op(ss.mean((2, 3))).mean(1)
        vals.append(op((ss if l == LEVELS - 1 else cs).mean((2, 3))))
        if l + 1 < LEVELS:
            pad = [xm.shape[2] % 2, xm.shape[3] % 2]
            xm, ym = op(F.avg_pool2d(xm, 2, padding=pad)), op(F.avg_pool2d(ym, 2, padding=pad))
    w = torch.tensor([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=dtype, device=x.device)
    ms = op(op(op(torch.stack(vals, -1).clamp(min=0)) ** w).prod(-1)).mean(1)
    return ssim.view(r, b), ms.view(r, b)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 3) for t in times]


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--no-eval", action="store_true")
    a = ap.parse_args()
    from wu import _lib, paired
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.from_numpy(paired.gaussian_window(K)).to(dev)
    for name in a.config:
        r, b, size, dt, vr = CONFIGS[name]
        gen = torch.Generator().manual_seed(0)
        x = torch.rand((b, 3, size, size), generator=gen) * 2 - 1
        y = (x.unsqueeze(0) * 0.9 + 0.1 * torch.randn((r, b, 3, size, size), generator=gen)).clamp(-1, 1)
        if dt == torch.uint8:
            x = ((x + 1) * 127.5).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
            y = ((y + 1) * 127.5).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous().to(dev).permute(0, 1, 4, 2, 3)
        else:
            x, y = x.to(dev, dt), y.to(dev, dt)
        scale, shift, L = paired.range_mapping(vr)

        def fused():
            st = paired.pair_stats(x, y, vr, K, levels=LEVELS)
            return paired.combine_ssim(st), paired.combine_ms_ssim(st)

        out = {"config": name, "R": r, "B": b, "size": size, "dtype": str(dt).split(".")[-1], "k": K, "levels": LEVELS, "steps": a.steps,
               "warmup": a.warmup, "fused_launches": 2 * LEVELS, "workspace_bytes": lib.wu_ssim_workspace_bytes(b, r, 3, size, size, K, LEVELS)}
        ms, all_ms = timed(fused, a.steps, a.warmup)
        out.update(fused_ms_median=round(ms, 3), fused_ms_all=all_ms, fused_peak_extra_bytes=peak_extra(fused))
        ref_s, ref_m = fused()
        for tag, cdt in (("fp64", torch.float64), ("fp32", torch.float32)):
            comp = lambda: composition(x, y, cdt, scale, shift, L, g)      # noqa: E731
            OPS[0] = 0
            s, m = comp()
            out[f"torch_{tag}_op_calls"] = OPS[0]
            ms, all_ms = timed(comp, a.steps, a.warmup)
            out[f"torch_{tag}_ms_median"], out[f"torch_{tag}_ms_all"] = round(ms, 3), all_ms
            out[f"torch_{tag}_peak_extra_bytes"] = peak_extra(comp)
            out[f"torch_{tag}_ssim_max_abs_diff"] = float((s.double() - ref_s).abs().max())
            out[f"torch_{tag}_ms_ssim_max_abs_diff"] = float((m.double() - ref_m).abs().max())
            del s, m
        out["ssim_mean"], out["ms_ssim_mean"] = float(ref_s.mean()), float(ref_m.mean())
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)
        del x, y
        torch.cuda.empty_cache()
    if not a.no_eval:
        import cunet
        from wu.evaluate import ClassTransferEval, ContentPreservation
        from wu.train_step import StandInEstimator
        nc, b, size = 5, 16, 224
        torch.manual_seed(0)
        net = cunet.Conditional_UNet(nc, precision="bf16").to(dev).eval()
        cls = StandInEstimator(nc).to(dev).eval()
        batch = (torch.rand((b, 3, size, size)) * 2 - 1).to(dev)
        plain = ClassTransferEval(net, cls, nc)
        with_c = ClassTransferEval(net, cls, nc, content=ContentPreservation())
        t0, all0 = timed(lambda: plain.update(batch), a.steps, a.warmup)
        t1, all1 = timed(lambda: with_c.update(batch), a.steps, a.warmup)
        fakes = net.sweep(batch, torch.eye(nc, device=dev), plain.max_images)
        t2, all2 = timed(lambda: with_c.content.add(batch, fakes), a.steps, a.warmup)
        print(json.dumps({"config": "ClassTransferEval.update", "classes": nc, "B": b, "size": size, "fakes_dtype": str(fakes.dtype),
                          "update_ms_median": round(t0, 3), "update_ms_all": all0, "update_with_content_ms_median": round(t1, 3),
                          "update_with_content_ms_all": all1, "content_add_alone_ms_median": round(t2, 3), "content_add_alone_ms_all": all2,
                          "share_of_update_with_content": round((t1 - t0) / t1, 4)}), flush=True)


if __name__ == "__main__":
    main()
