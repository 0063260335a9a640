"""Device time and peak memory of the colour-transfer baseline (wu.colour -> csrc/colour_ot.hip) against the composition of the same numbers
out of torch ops on the same GPU: float64 matmul projection, torch.sort, torch.searchsorted left and right, gather, matmul back, update.

    python scratch/bench_colour.py [--steps 5] [--warmup 2] [--cases eval,eval_k1,sweep512,u8_256] [--no-eval-share]

  eval      the evaluation sweep: R = 5 targets, B = 16, 224 x 224, P = 65 536, K = 20, bf16 input
  eval_k1   the same with K = 1 (per-channel histogram matching)
  sweep512  the class sweep at 512 x 512, B = 16, R = 5, K = 20, bf16
  u8_256    64 uint8 photographs (NHWC views) at 256 x 256 to one class, K = 20

One JSON line per case: medians over the timed calls (device events around one whole call, inputs resident; the two sides alternate call by
call), all the times, the peak device memory above the resident inputs, the largest difference of the two results (the composition's
matmuls fuse and reorder, so it is not bit-equal), and the split of ONE iteration of wu_colour_ot_step into the existing sort
(wu_swd_sort_columns on keys of the same shape, its input copy subtracted) and the rest: the new projection and fused match kernels.  A last
line gives the share of a ClassTransferEval.update (ResNet-101 classifier, SSIM content metric) that the baseline's sweep takes, next to the
generator's sweep of the same batch."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = {"eval": (5, 16, 224, 65536, 20, "bf16"), "eval_k1": (5, 16, 224, 65536, 1, "bf16"), "sweep512": (5, 16, 512, 65536, 20, "bf16"),
         "u8_256": (1, 64, 256, 65536, 20, "u8")}
NC = 5


def timed_pair(fa, fb, steps, warmup):
    """Medians of fa and fb, timed alternately."""
    for _ in range(warmup):
        fa()
        if fb is not None:
            fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        for fn, acc in ((fa, ta), (fb, tb)):
            if fn is None:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1))
    med = lambda t: round(float(np.median(t)), 3) if t else None  # noqa: E731
    return med(ta), [round(t, 3) for t in ta], med(tb), [round(t, 3) for t in tb]


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def torch_transfer(x, pal, targets, rots, step, value_range):
    """The same numbers out of torch ops: (R, B, 3, H, W) of x's dtype."""
    from wu import paired
    scale, shift, L = paired.range_mapping(value_range)
    b, _, h, w = x.shape
    n, r, P = h * w, len(targets), pal.shape[1]
    s = ((x.double() * scale + shift) / L).reshape(1, b, 3, n).expand(r, b, 3, n).reshape(r * b, 3, n).clone()
    base = (torch.tensor(targets, device=x.device).repeat_interleave(b).view(-1, 1, 1) * 3 + torch.arange(3, device=x.device).view(1, 3, 1)) * P
    palT = pal.transpose(1, 2)
    for R in rots:
        Rt = torch.from_numpy(R).to(x.device)
        keys = torch.matmul(Rt, s)
        q = torch.sort(torch.matmul(Rt, palT), dim=2)[0].reshape(-1)
        srt = torch.sort(keys, dim=2)[0]
        lo = torch.searchsorted(srt, keys, right=False)
        hi = torch.searchsorted(srt, keys, right=True)
        t = ((lo + hi) * P) // (2 * n)
        delta = q[base + t] - keys
        s = s + step * torch.matmul(Rt.t(), delta)
    u = s.clamp(0, 1)
    if isinstance(value_range, str):
        v = torch.round(u * 255)
    else:
        v = value_range[0] + u * (value_range[1] - value_range[0])
    if x.dtype == torch.uint8:
        v = torch.round(v)
    return v.to(torch.float32).to(x.dtype).view(r, b, 3, h, w)


def make_input(b, size, kind, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    coarse = torch.rand((b, size // 8, size // 8, 3), generator=gen, device=dev)
    x = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2) * 0.6 + 0.4 * torch.rand((b, size, size, 3), generator=gen, device=dev)
    if kind == "u8":
        return (x * 255).round().to(torch.uint8).permute(0, 3, 1, 2), "uint8"           # NHWC storage, read through its strides
    x = (x * 2 - 1).permute(0, 3, 1, 2).contiguous()
    return (x.to(torch.bfloat16) if kind == "bf16" else x), (-1, 1)


def make_palettes(P, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    mean = torch.rand((NC, 1, 3), generator=gen, device=dev, dtype=torch.float64) * 0.6 + 0.2
    return (mean + 0.15 * torch.randn((NC, P, 3), generator=gen, device=dev, dtype=torch.float64)).clamp(0, 1)


def step_split(nimg, n, P, pal, steps, warmup):
    """One iteration through the ABI, and the existing sort on keys of the same shape."""
    from wu import _lib, colour, swd
    from wu.layout import stream_ptr
    lib = _lib.load()
    dev = pal.device
    rot = colour.draw_rotations(0, 2)[1]
    rot_c = (ctypes.c_double * 9)(*rot.reshape(-1).tolist())
    ws = torch.empty(lib.wu_colour_ot_workspace_bytes(nimg, n, NC, P), dtype=torch.uint8, device=dev)
    state0 = torch.rand((nimg, 3, n), dtype=torch.float64, device=dev)
    state = state0.clone()
    keys = torch.empty((NC * 3, P), dtype=torch.float64, device=dev)
    cls = (torch.arange(nimg, device=dev) % NC).to(torch.int32)
    _lib.call("wu_colour_ot_palette_keys", pal.data_ptr(), NC, P, rot_c, keys.data_ptr(), ws.data_ptr(), stream_ptr())

    def one_step():
        state.copy_(state0)
        _lib.call("wu_colour_ot_step", state.data_ptr(), nimg, n, keys.data_ptr(), NC, P, cls.data_ptr(), rot_c, 1.0, ws.data_ptr(), stream_ptr())

    def pal_keys():
        _lib.call("wu_colour_ot_palette_keys", pal.data_ptr(), NC, P, rot_c, keys.data_ptr(), ws.data_ptr(), stream_ptr())

    copy_ms = timed_pair(lambda: state.copy_(state0), None, steps, warmup)[0]
    step_ms = timed_pair(one_step, None, steps, warmup)[0] - copy_ms
    pal_ms = timed_pair(pal_keys, None, steps, warmup)[0]
    # the sort alone, in groups of at most 4095 columns as the step makes them
    chunk = max(1, min(nimg, 4096 // 3, (256 << 20) // (3 * n * 8)))
    sort_ms = 0.0
    for v0 in range(0, nimg, chunk):
        k = min(chunk, nimg - v0)
        src = state0[v0:v0 + k].reshape(3 * k, n)
        work = src.clone()

        def srt():
            work.copy_(src)
            swd.sort_columns(work)

        c_ms = timed_pair(lambda: work.copy_(src), None, steps, warmup)[0]
        sort_ms += timed_pair(srt, None, steps, warmup)[0] - c_ms
    return {"one_step_ms": round(step_ms, 3), "of_which_existing_sort_ms": round(sort_ms, 3),
            "new_project_and_match_ms": round(step_ms - sort_ms, 3), "palette_keys_ms": round(pal_ms, 3), "images_per_sort": chunk}


def bench_case(name, a, dev):
    from wu import colour
    r, b, size, P, K, kind = CASES[name]
    x, value_range = make_input(b, size, kind, dev, seed=1)
    pal_t = make_palettes(P, dev)
    pal = colour.ClassPalettes(pal_t)
    targets = list(range(r)) if r > 1 else [2]
    rots = colour.draw_rotations(0, K)

    def fused():
        return colour.transfer(x, pal, targets, K, 0, 1.0, value_range)

    def comp():
        return torch_transfer(x, pal_t, targets, rots, 1.0, value_range)

    out = {"case": name, "R": r, "B": b, "size": size, "P": P, "K": K, "dtype": str(x.dtype), "steps": a.steps, "warmup": a.warmup}
    got, ref = fused(), comp()
    diff = (got.float() - ref.float()).abs()
    out["max_abs_diff_vs_torch"] = float(diff.max())
    out["values_that_differ"] = int((diff > 0).sum())
    out["values"] = diff.numel()
    del got, ref, diff
    fm, fall, tm, tall = timed_pair(fused, comp, a.steps, a.warmup)
    out.update(fused_ms_median=fm, fused_ms_all=fall, torch_ms_median=tm, torch_ms_all=tall, torch_over_fused=round(tm / fm, 3))
    out["fused_peak_extra_bytes"] = peak_extra(fused)
    out["torch_peak_extra_bytes"] = peak_extra(comp)
    out["split"] = step_split(r * b, size * size, P, pal_t, a.steps, a.warmup)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def bench_eval_share(a, dev):
    """ClassTransferEval.update with the baseline as its transfer, and the generator's sweep of the same batch."""
    import cunet
    from wu import colour, evaluate
    from wu.resnet import ResNet101Estimator
    torch.manual_seed(0)
    x, _ = make_input(16, 224, "f32", dev, seed=2)
    pal = colour.ClassPalettes(make_palettes(65536, dev))
    clf = ResNet101Estimator(NC, precision="bf16").to(dev).eval()
    net = cunet.Conditional_UNet(NC, precision="bf16").to(dev).eval()
    base = colour.ColourBaseline(pal, iters=20)
    rows = torch.eye(NC, device=dev)
    ev = evaluate.ClassTransferEval(base, clf, NC, content=evaluate.ContentPreservation(ms=True))
    with torch.no_grad():
        sweep_b, _, sweep_g, _ = timed_pair(lambda: base.sweep(x, rows, evaluate.SWEEP_MAX_IMAGES),
                                            lambda: net.sweep(x, rows, evaluate.SWEEP_MAX_IMAGES), a.steps, a.warmup)
        upd, upd_all, _, _ = timed_pair(lambda: ev.update(x), None, a.steps, a.warmup)
    print(json.dumps({"case": "eval_share", "B": 16, "size": 224, "R": NC, "K": 20, "P": 65536, "dtype": "float32",
                      "baseline_sweep_ms": sweep_b, "generator_sweep_ms": sweep_g, "update_with_baseline_ms": upd, "update_ms_all": upd_all,
                      "baseline_share_of_update": round(sweep_b / upd, 3), "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-eval-share", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_colour.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for name in a.cases.split(","):
        bench_case(name, a, dev)
        torch.cuda.empty_cache()
    if not a.no_eval_share:
        bench_eval_share(a, dev)


if __name__ == "__main__":
    main()
