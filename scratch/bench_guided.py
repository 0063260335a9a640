"""Device time of the fused full-resolution path (wu.guided.GuidedUpsampler: wu_guided_coeffs, 5 launches at r = 4, + wu_guided_apply, 1 launch;
csrc/guided.hip) against the torch composition of the same numbers on the same GPU: avg_pool2d(count_include_pad=False) boxes, the
closed-form 3 x 3 inverse, F.interpolate(bilinear, align_corners=False) of the twelve coefficient maps, multiply-add -- once with float64
maps and once with float32 maps.

    python scratch/bench_guided.py [--steps 10] [--warmup 3] [--config flickr big1 big5 year e2e] [--out FILE]

  flickr  N = 64 photographs of 500 x 375, S = 224, R = 5            (the Flickr batch under the class sweep)
  big1    N = 16 photographs of 4000 x 3000, S = 256, R = 1
  big5    the same, R = 5
  year    N = 1, 1024 x 768, S = 224, R = 365 in chunks of 73 rows   (a year of signals)
  e2e     fullres_sweep_to_dir against class_sweep_to_dir on the same 16 JPEG files of 500 x 375 (decode and input pipeline included in
          both): what full resolution costs, host clock around calls that end with the files written

Per config one JSON line: the median of the timed calls (device events around one whole call, inputs resident, output allocation included)
of the fused path, of its two stages alone and of the two compositions; peak extra device memory of each (torch.cuda.max_memory_allocated
above what was resident); for the apply stage the bytes and float64 operations the algorithm needs (counted from the formulas, not
measured) over its time; how far the compositions' bytes lie from the fused ones.  The compositions hold the full-resolution maps of at most
MAP_BUDGET bytes at a time (they walk the (row, image) pairs in chunks), or the big configs would not fit in memory at all."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda:0"
CONFIGS = {"flickr": (64, 375, 500, 224, 5, 5), "big1": (16, 3000, 4000, 256, 1, 1), "big5": (16, 3000, 4000, 256, 5, 5),
           "year": (1, 768, 1024, 224, 365, 73)}                    # N, h, w, S, R, rows per call
R_, EPS = 4, 1e-3
MAP_BUDGET = 4 << 30
HBM_RATE, F64_RATE = 8.0e12, 78.6e12                                # datasheet: HBM3E bytes / s, vector float64 FLOP / s (FMA = 2)
OPS_PER_PIXEL = 12 * 9 + 3 * 6 + 3 * 3                              # 12 bilinear taps of 9 operations, 3 x (3 mul + 3 add), x 255 and two clamps


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
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def inverse3(S):
    """Closed-form inverse of symmetric 3 x 3 matrices given as the six maps (00, 01, 02, 11, 12, 22)."""
    a, b, c, d, e, f = S
    c00, c01, c02, c11, c12, c22 = d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    i = [v / det for v in (c00, c01, c02, c11, c12, c22)]
    return [[i[0], i[1], i[2]], [i[1], i[3], i[4]], [i[2], i[4], i[5]]]


def composition(guide, low, photos, dtype):
    """(R, N, h, w, 3) uint8 by torch ops with `dtype` maps; all photographs of one size."""
    r, n, _, s, _ = low.shape
    h, w = photos.shape[1:3]
    k = 2 * R_ + 1

    def box(v):
        return F.avg_pool2d(v, k, 1, R_, count_include_pad=False)

    I = guide.to(dtype) * 0.5 + 0.5
    mI = box(I)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    S = [box(I[:, j] * I[:, kk]) - mI[:, j] * mI[:, kk] + (EPS if j == kk else 0.0) for j, kk in pairs]
    inv = inverse3(S)
    p = low.to(dtype)
    bp = box(p.flatten(0, 1)).view(r, n, 3, s, s)
    coef = torch.empty(r, n, 12, s, s, dtype=dtype, device=guide.device)
    for c in range(3):
        cov = [box((I[:, kk] * p[:, :, c]).reshape(r * n, 1, s, s)).view(r, n, s, s) - mI[:, kk] * bp[:, :, c] for kk in range(3)]
        a = [inv[kk][0] * cov[0] + inv[kk][1] * cov[1] + inv[kk][2] * cov[2] for kk in range(3)]
        b = bp[:, :, c] - (a[0] * mI[:, 0] + a[1] * mI[:, 1] + a[2] * mI[:, 2])
        for kk in range(3):
            coef[:, :, 3 * c + kk] = a[kk]
        coef[:, :, 9 + c] = b
    coef = box(coef.view(r * n, 12, s, s))
    out = torch.empty(r * n, h, w, 3, dtype=torch.uint8, device=guide.device)
    Ih = photos.permute(0, 3, 1, 2).to(dtype) / 255.0                                   # (N, 3, h, w)
    chunk = max(1, int(MAP_BUDGET // (12 * h * w * coef.element_size())))
    for at in range(0, r * n, chunk):
        full = F.interpolate(coef[at:at + chunk], size=(h, w), mode="bilinear", align_corners=False)
        idx = torch.arange(at, min(at + chunk, r * n), device=guide.device) % n
        ih = Ih[idx]
        q = torch.stack([full[:, 3 * c] * ih[:, 0] + full[:, 3 * c + 1] * ih[:, 1] + full[:, 3 * c + 2] * ih[:, 2] + full[:, 9 + c]
                         for c in range(3)], -1)
        out[at:at + chunk] = q.mul_(255).clamp_(0, 255).to(torch.uint8)
    return out.view(r, n, h, w, 3)


def make_inputs(n, h, w, s, r, seed=0):
    from wu.input_pipeline import GPUInputPipeline
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand((n, 3, (h + 7) // 8, (w + 7) // 8), generator=g, device=DEV)
    photos = (F.interpolate(coarse, size=(h, w), mode="nearest") * 180 + torch.rand((n, 3, h, w), generator=g, device=DEV) * 75)
    photos = photos.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    sizes = [(h, w)] * n
    guide = GPUInputPipeline(s, train=False)(photos, sizes)
    mix = torch.rand((r, 3, 3), generator=g, device=DEV) * 0.5
    low = (torch.einsum("rck,nkhw->rnchw", mix, guide * 0.5 + 0.5) * 0.6 + torch.rand((r, n, 3, s, s), generator=g, device=DEV) * 0.1).clamp_(0, 1)
    low = low.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)                 # channels-last, as the sweep returns it
    return photos, sizes, guide, low


def run_config(name, steps, warmup):
    from wu import _lib
    from wu.guided import GuidedUpsampler
    n, h, w, s, r, per_call = CONFIGS[name]
    photos, sizes, guide, low = make_inputs(n, h, w, s, r)
    up = GuidedUpsampler(R_, EPS)
    chunks = [(at, min(at + per_call, r)) for at in range(0, r, per_call)]

    def fused():
        return [up.upsample(guide, low[a:b], photos, sizes) for a, b in chunks]

    def coeffs_only():
        return [up.coefficients(guide, low[a:b]) for a, b in chunks]

    co = coeffs_only()

    def apply_only():
        return [up.apply(c, photos, sizes) for c in co]

    res = {"config": name, "N": n, "h": h, "w": w, "S": s, "R": r, "rows_per_call": per_call, "r": R_, "eps": EPS,
           "launches_per_call": 6, "workspace_bytes": int(_lib.load().wu_guided_workspace_bytes(n, per_call, s, s)),
           "coeff_bytes_per_call": per_call * n * 12 * s * s * 8}
    res["fused_ms"], res["fused_all"] = timed(fused, steps, warmup)
    res["fused_peak_extra"] = peak_extra(fused)
    res["coeffs_ms"], _ = timed(coeffs_only, steps, warmup)
    res["apply_ms"], _ = timed(apply_only, steps, warmup)
    px = n * h * w
    res["apply_bytes"] = px * 3 + r * px * 3 + r * n * 12 * s * s * 8
    res["apply_flops"] = r * px * OPS_PER_PIXEL
    res["apply_bytes_per_s"] = res["apply_bytes"] / (res["apply_ms"] * 1e-3)
    res["apply_flops_per_s"] = res["apply_flops"] / (res["apply_ms"] * 1e-3)
    res["apply_share_of_hbm"] = res["apply_bytes_per_s"] / HBM_RATE
    res["apply_share_of_f64"] = res["apply_flops_per_s"] / F64_RATE
    want = torch.cat(fused())
    del co
    for label, dtype in (("torch64", torch.float64), ("torch32", torch.float32)):
        def comp():
            return [composition(guide, low[a:b], photos, dtype) for a, b in chunks]
        try:
            res[label + "_ms"], _ = timed(comp, steps, warmup)
            res[label + "_peak_extra"] = peak_extra(comp)
            d = (torch.cat(comp()).to(torch.int16) - want.to(torch.int16)).abs()
            res[label + "_bytes_differ"] = float((d > 0).float().mean())
            res[label + "_max_byte_diff"] = int(d.max())
            del d
        except torch.cuda.OutOfMemoryError as e:                    # a loss of the composition, reported as such
            res[label + "_ms"] = None
            res[label + "_error"] = str(e).splitlines()[0]
        torch.cuda.empty_cache()
    return res


def run_e2e(steps, warmup):
    """Host clock: both drivers from the same JPEG files to files on disk."""
    from PIL import Image
    import cunet
    from wu import infer_driver as D
    from wu.input_pipeline import GPUInputPipeline
    from wu.jpeg import GPUJpegDecoder
    n, h, w, s, nc = 16, 375, 500, 224, 5
    names = [f"c{i}" for i in range(nc)]
    torch.manual_seed(0)
    net = cunet.Conditional_UNet(nc, precision="bf16").to(DEV).eval()
    photos, _, _, _ = make_inputs(n, h, w, s, 1, seed=1)
    tmp = tempfile.mkdtemp(prefix="bench_guided_")
    files = []
    for i, img in enumerate(photos.cpu().numpy()):
        files.append(os.path.join(tmp, f"im{i:03d}.jpg"))
        Image.fromarray(img).save(files[-1], quality=90)
    dec = GPUJpegDecoder()
    labels = [i % nc for i in range(n)]

    def low_res():
        ph, sizes = dec.decode_batch(files)
        batch = GPUInputPipeline(s, train=False)(ph, sizes)
        return D.class_sweep_to_dir(net, batch, [f"im{i:03d}" for i in range(n)], labels, names, os.path.join(tmp, "low"), shared_encoder=True)

    def full_res():
        return D.fullres_sweep_to_dir(net, files, labels, names, os.path.join(tmp, "full"), input_size=s, decoder=dec)

    out = {"config": "e2e", "N": n, "h": h, "w": w, "S": s, "classes": nc}
    for label, fn in (("class_sweep_to_dir", low_res), ("fullres_sweep_to_dir", full_res)):
        for _ in range(warmup):
            fn()
        times = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            written = fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[label + "_ms"] = float(np.median(times))
        out[label + "_all"] = [round(t, 2) for t in times]
        out[label + "_file_bytes"] = sum(os.path.getsize(p) for p in written)
    dec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", nargs="+", default=["flickr", "big1", "big5", "year", "e2e"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided.py needs the GPU: no CPU timing is meaningful")
    for name in args.config:
        res = run_e2e(args.steps, args.warmup) if name == "e2e" else run_config(name, args.steps, args.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
