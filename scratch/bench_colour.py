"""Device time and peak memory of the colour-transfer baseline (wu.colour -> csrc/colour_ot.hip) against the composition of the same numbers
out of torch ops on the same GPU: float64 matmul projection, torch.sort, torch.searchsorted left and right, gather, matmul back, update.

    python scratch/bench_colour.py [--steps 5] [--warmup 2] [--cases eval,eval_k1,sweep512,u8_256] [--no-eval-share]
                                   [--extra regrain,linear] [--extra-cases eval,sweep512,u8_256]

  eval      the evaluation sweep: R = 5 targets, B = 16, 224 x 224, P = 65 536, K = 20, bf16 input
  eval_k1   the same with K = 1 (per-channel histogram matching)
  sweep512  the class sweep at 512 x 512, B = 16, R = 5, K = 20, bf16
  u8_256    64 uint8 photographs (NHWC views) at 256 x 256 to one class, K = 20

One JSON line per case: medians over the timed calls (device events around one whole call, inputs resident; the two sides alternate call by
call), all the times, the peak device memory above the resident inputs, the largest difference of the two results (the composition's
matmuls fuse and reorder, so it is not bit-equal), and the split of ONE iteration of wu_colour_ot_step into the existing sort
(wu_swd_sort_columns on keys of the same shape, its input copy subtracted) and the rest: the new projection and fused match kernels.  A last
line gives the share of a ClassTransferEval.update (ResNet-101 classifier, SSIM content metric) that the baseline's sweep takes, next to the
generator's sweep of the same batch.

--extra regrain: per case, wu.colour.regrain alone and transfer(..., regrain=True) against the torch composition of the regraining rule
(float64 tensors, clamped index gathers, one op per term), with the launch count of the shipped solve.  --extra linear: method="meanstd" /
"mkl" against torch (mean, centred matmul, torch.linalg.eigh).  With an --extra the eval-share line also carries the share of every method,
with and without regraining."""
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


def _sh(a, dy, dx):
    h, w = a.shape[-2:]
    y = (torch.arange(h, device=a.device) + dy).clamp(0, h - 1)
    x = (torch.arange(w, device=a.device) + dx).clamp(0, w - 1)
    return a[..., y[:, None], x[None, :]]


def _down(a):
    for ax in (-2, -1):
        n = a.shape[ax]
        d = torch.arange((n + 1) // 2, device=a.device)
        a = (a.index_select(ax % a.dim(), 2 * d) + a.index_select(ax % a.dim(), (2 * d + 1).clamp(max=n - 1))) * 0.5
    return a


def _up(a, h, w):
    for ax, n in ((-2, h), (-1, w)):
        nc = a.shape[ax]
        d = torch.arange(n, device=a.device)
        o = torch.where(d % 2 == 0, d // 2 - 1, d // 2 + 1).clamp(0, nc - 1)
        a = a.index_select(ax % a.dim(), d // 2) * 0.75 + a.index_select(ax % a.dim(), o) * 0.25
    return a


NBRS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def torch_regrain_state(i0, it, iters, smoothness, min_side):
    """The regraining rule out of torch ops on (N, 3, h, w) float64 states."""
    def rec(ir, i0, it, level, levels):
        if level + 1 < levels:
            c0 = _down(ir)
            c1 = rec(c0, _down(i0), _down(it), level + 1, levels)
            ir = ir + _up(c1 - c0, ir.shape[-2], ir.shape[-1])
        gx, gy = _sh(i0, 0, 1) - _sh(i0, 0, -1), _sh(i0, 1, 0) - _sh(i0, -1, 0)
        q = gx * gx + gy * gy
        dI = torch.sqrt((q[:, 0] + q[:, 1]) + q[:, 2]).unsqueeze(1)
        psi = ((256.0 * dI) / 5.0).clamp(max=1.0)
        phi = (30.0 * 2.0 ** -level) / (1.0 + (10.0 * dI) / smoothness)
        pj = [(_sh(phi, dy, dx) + phi) * 0.5 for dy, dx in NBRS]
        den = ((((psi + pj[0]) + pj[1]) + pj[2]) + pj[3]) + 2.0 ** -52
        b = psi * it
        for j, (dy, dx) in enumerate(NBRS):
            b = b + pj[j] * (i0 - _sh(i0, dy, dx))
        for _ in range(iters[level]):
            a = b
            for j, (dy, dx) in enumerate(NBRS):
                a = a + pj[j] * _sh(ir, dy, dx)
            ir = (a / den) * 0.8 + 0.2 * ir
        return ir

    h, w = i0.shape[-2:]
    levels = 1
    while levels < len(iters) and (h + 1) // 2 > min_side and (w + 1) // 2 > min_side:
        h, w, levels = (h + 1) // 2, (w + 1) // 2, levels + 1
    return rec(it, i0, it, 0, levels)


def _to_state(x, value_range):
    from wu import paired
    scale, shift, L = paired.range_mapping(value_range)
    return (x.double() * scale + shift) / L


def _from_state(s, value_range, dtype):
    u = s.clamp(0, 1)
    v = torch.round(u * 255) if isinstance(value_range, str) else value_range[0] + u * (value_range[1] - value_range[0])
    if dtype == torch.uint8:
        v = torch.round(v)
    return v.to(torch.float32).to(dtype)


def torch_regrain(x, y, value_range, iters=(4, 16, 32, 64, 64, 64), smoothness=1.0, min_side=20):
    """x (B, 3, H, W), y (R, B, 3, H, W) -> y's shape and dtype."""
    r, b = y.shape[:2]
    i0 = _to_state(x, value_range).unsqueeze(0).expand(r, *x.shape).reshape(r * b, *x.shape[1:])
    it = _to_state(y, value_range).reshape(r * b, *x.shape[1:])
    return _from_state(torch_regrain_state(i0, it, iters, smoothness, min_side), value_range, y.dtype).view(y.shape)


def torch_linear(x, pal, targets, method, value_range, eps=1e-10):
    """mean / sigma transfer or the Monge-Kantorovich map out of torch ops: (R, B, 3, H, W) of x's dtype."""
    b, _, h, w = x.shape
    r = len(targets)
    s = _to_state(x, value_range).reshape(b, 3, h * w)
    mu_s = s.mean(2, keepdim=True)
    d = s - mu_s
    cs = torch.matmul(d, d.transpose(1, 2)) / (h * w)
    pt = pal[torch.tensor(targets, device=x.device)].transpose(1, 2)          # (R, 3, P)
    mu_t = pt.mean(2, keepdim=True)
    dt = pt - mu_t
    ct = torch.matmul(dt, dt.transpose(1, 2)) / pt.shape[2]
    if method == "meanstd":
        A = torch.diag_embed(torch.sqrt(torch.diagonal(ct, dim1=1, dim2=2)[:, None] / torch.diagonal(cs, dim1=1, dim2=2)[None].clamp(min=eps)))
    else:
        lam, V = torch.linalg.eigh(cs)
        f = lam.clamp(min=eps).sqrt()
        S = torch.matmul(V * f[:, None, :], V.transpose(1, 2))
        Si = torch.matmul(V / f[:, None, :], V.transpose(1, 2))
        M = torch.matmul(torch.matmul(S[None], ct[:, None]), S[None])           # (R, B, 3, 3)
        lm, U = torch.linalg.eigh(M)
        Mr = torch.matmul(U * lm.clamp(min=0).sqrt()[..., None, :], U.transpose(-1, -2))
        A = torch.matmul(torch.matmul(Si[None], Mr), Si[None])
    out = torch.matmul(A, d[None]) + mu_t[:, None]
    return _from_state(out, value_range, x.dtype).view(r, b, 3, h, w)


def solve_launches(h, w, iters=(4, 16, 32, 64, 64, 64), min_side=20, region=4096, max_t=8):
    """Launches of regrain_solve_kernel, and the Jacobi iterations they cover (= launches at one launch per iteration)."""
    launches = total = 0
    for level, k in enumerate(iters):
        total += k
        launches += 1 if h * w <= region else -(-k // max_t)
        if level + 1 == len(iters) or (h + 1) // 2 <= min_side or (w + 1) // 2 <= min_side:
            break
        h, w = (h + 1) // 2, (w + 1) // 2
    return launches, total


def bench_extra(name, a, dev, what):
    from wu import colour
    r, b, size, P, K, kind = CASES[name]
    x, value_range = make_input(b, size, kind, dev, seed=1)
    pal_t = make_palettes(P, dev)
    pal = colour.ClassPalettes(pal_t)
    targets = list(range(r)) if r > 1 else [2]
    base = {"case": name, "R": r, "B": b, "size": size, "P": P, "dtype": str(x.dtype), "steps": a.steps, "warmup": a.warmup,
            "device": torch.cuda.get_device_name(0)}
    if "regrain" in what:
        y = colour.transfer(x, pal, targets, K, 0, 1.0, value_range)
        got, ref = colour.regrain(x, y, value_range), torch_regrain(x, y, value_range)
        diff = (got.float() - ref.float()).abs()
        out = dict(base, what="regrain alone", max_abs_diff_vs_torch=float(diff.max()), values_that_differ=int((diff > 0).sum()))
        del got, ref, diff
        fm, fall, tm, tall = timed_pair(lambda: colour.regrain(x, y, value_range), lambda: torch_regrain(x, y, value_range), a.steps, a.warmup)
        out.update(fused_ms_median=fm, fused_ms_all=fall, torch_ms_median=tm, torch_ms_all=tall, torch_over_fused=round(tm / fm, 3))
        out["fused_peak_extra_bytes"] = peak_extra(lambda: colour.regrain(x, y, value_range))
        out["torch_peak_extra_bytes"] = peak_extra(lambda: torch_regrain(x, y, value_range))
        out["solve_launches"], out["jacobi_iterations"] = solve_launches(size, size)
        print(json.dumps(out), flush=True)
        pm, pall, rm, rall = timed_pair(lambda: colour.transfer(x, pal, targets, K, 0, 1.0, value_range),
                                        lambda: colour.transfer(x, pal, targets, K, 0, 1.0, value_range, regrain=True), a.steps, a.warmup)
        print(json.dumps(dict(base, what="transfer idt", K=K, plain_ms_median=pm, plain_ms_all=pall, regrain_ms_median=rm, regrain_ms_all=rall,
                              regrain_peak_extra_bytes=peak_extra(lambda: colour.transfer(x, pal, targets, K, 0, 1.0, value_range, regrain=True)),
                              plain_peak_extra_bytes=peak_extra(lambda: colour.transfer(x, pal, targets, K, 0, 1.0, value_range)))), flush=True)
        del y
    if "linear" in what:
        for method in ("meanstd", "mkl"):
            fused = lambda: colour.transfer(x, pal, targets, value_range=value_range, method=method)  # noqa: E731
            comp = lambda: torch_linear(x, pal_t, targets, method, value_range)  # noqa: E731
            diff = (fused().float() - comp().float()).abs()
            out = dict(base, what=method, max_abs_diff_vs_torch=float(diff.max()), values_that_differ=int((diff > 0).sum()))
            del diff
            fm, fall, tm, tall = timed_pair(fused, comp, a.steps, a.warmup)
            out.update(fused_ms_median=fm, fused_ms_all=fall, torch_ms_median=tm, torch_ms_all=tall, torch_over_fused=round(tm / fm, 3))
            out["fused_peak_extra_bytes"], out["torch_peak_extra_bytes"] = peak_extra(fused), peak_extra(comp)
            out["with_regrain_ms_median"] = timed_pair(lambda: colour.transfer(x, pal, targets, value_range=value_range, method=method,
                                                                               regrain=True), None, a.steps, a.warmup)[0]
            print(json.dumps(out), flush=True)


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
    """ClassTransferEval.update with the baseline as its transfer, and the generator's sweep of the same batch.

--extra regrain: per case, wu.colour.regrain alone and transfer(..., regrain=True) against the torch composition of the regraining rule
(float64 tensors, clamped index gathers, one op per term), with the launch count of the shipped solve.  --extra linear: method="meanstd" /
"mkl" against torch (mean, centred matmul, torch.linalg.eigh).  With an --extra the eval-share line also carries the share of every method,
with and without regraining."""
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
    if not a.extra:
        return
    for method in ("idt", "meanstd", "mkl"):
        for rg in (None, True):
            bl = colour.ColourBaseline(pal, iters=20, method=method, regrain=rg)
            ev = evaluate.ClassTransferEval(bl, clf, NC, content=evaluate.ContentPreservation(ms=True))
            with torch.no_grad():
                sw = timed_pair(lambda: bl.sweep(x, rows, evaluate.SWEEP_MAX_IMAGES), None, a.steps, a.warmup)[0]
                up = timed_pair(lambda: ev.update(x), None, a.steps, a.warmup)[0]
            print(json.dumps({"case": "eval_share", "method": method, "regrain": bool(rg), "sweep_ms": sw, "update_ms": up,
                              "share_of_update": round(sw / up, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-eval-share", action="store_true")
    ap.add_argument("--extra", default="", help="regrain,linear: the rows of the regraining pass and of the linear maps")
    ap.add_argument("--extra-cases", default="eval,sweep512,u8_256")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_colour.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for name in [c for c in a.cases.split(",") if c]:
        bench_case(name, a, dev)
        torch.cuda.empty_cache()
    if a.extra:
        for name in a.extra_cases.split(","):
            bench_extra(name, a, dev, a.extra.split(","))
            torch.cuda.empty_cache()
    if not a.no_eval_share:
        bench_eval_share(a, dev)


if __name__ == "__main__":
    main()
