"""Device time of the resampling front end (wu.resample.GPUResampler: ONE launch of resample_kernel, csrc/resample.hip) against two
baselines that do the same job, and its share of a ``python -m wu.fid --resize clean`` pass.

    python scratch/bench_resample.py [--steps 10] [--warmup 3] [--config flickr big_f32 big_u8 fid] [--out FILE]

  flickr   64 photographs of 500 x 375  -> 299 x 299, bicubic, float mode, epilogue clip / 255 (fp32 NCHW)
  big_f32  16 photographs of 4000 x 3000 -> 299 x 299, bicubic, float mode, the same epilogue
  big_u8   16 photographs of 4000 x 3000 -> 224 x 224, Lanczos, 8-bit mode, uint8 NHWC
  fid      fid.statistics_of_path over 100 PNG files of 500 x 375 with a randomly initialised InceptionV3, resize="clean" beside
           resize="legacy" on the same files (host clock around the whole pass: file reads and Pillow decode included in both), and
           the device time of the resampler alone on the same batches: its share of the clean pass

Baselines: ``F.interpolate(mode="bicubic", antialias=True)`` in fp32 on the same GPU from the same resident uint8 NHWC batch (the
permute + float conversion it needs is inside its timed window; it has no Lanczos, so big_u8 is compared with its bicubic; it gives nearly
the same numbers, not the same bits: the largest difference is reported), and Pillow's Image.resize on 16 host threads from host arrays
(float mode: three mode 'F' channels per image), host clock, no transfers.  The resampler's window holds the table look-up, the upload of
descriptors and tables, the launch and the output allocation: device events around one whole call, inputs resident.  One JSON line per
config; bytes and float64 operations are counted from the shapes (the algorithm's need: every source byte once, every tap one multiply
and one add per channel), not measured."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda:0"
CONFIGS = {"flickr": (64, 375, 500, 299, "bicubic", "f32"), "big_f32": (16, 3000, 4000, 299, "bicubic", "f32"),
           "big_u8": (16, 3000, 4000, 224, "lanczos", "u8")}
THREADS = 16
HBM_RATE, F64_RATE = 8.0e12, 78.6e12                                # datasheet: HBM3E bytes / s, vector float64 FLOP / s (FMA = 2)


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


def photographs(n, h, w, seed=0):
    """(n, h, w, 3) uint8 on the GPU: smooth regions plus noise, as a photograph has."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand((n, 3, (h + 7) // 8, (w + 7) // 8), generator=g, device=DEV)
    x = F.interpolate(coarse, size=(h, w), mode="nearest") * 180 + torch.rand((n, 3, h, w), generator=g, device=DEV) * 75
    return x.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def taps(in_size, out_size, filt):
    from wu.resample import coefficients
    return int(coefficients(in_size, out_size, filt)[0][:, 1].sum()) if in_size != out_size else 0


def run_config(name, steps, warmup):
    from PIL import Image
    from wu.resample import GPUResampler
    n, h, w, s, filt, mode = CONFIGS[name]
    photos = photographs(n, h, w)
    rs = GPUResampler(s, filt, mode, "nhwc_u8" if mode == "u8" else "unit")
    res = {"config": name, "N": n, "h": h, "w": w, "S": s, "filter": filt, "mode": mode, "launches_per_call": 1}
    res["resampler_ms"], res["resampler_all"] = timed(lambda: rs(photos), steps, warmup)
    # the algorithm's need: the horizontal pass over every source row, the vertical pass over s columns
    flops = n * 3 * 2 * (h * taps(w, s, filt) + s * taps(h, s, filt))
    res["bytes"] = n * h * w * 3 + n * s * s * 3 * (1 if mode == "u8" else 4)
    res["flops"] = flops
    res["bytes_per_s"] = res["bytes"] / (res["resampler_ms"] * 1e-3)
    res["flops_per_s"] = flops / (res["resampler_ms"] * 1e-3)
    res["share_of_hbm"] = res["bytes_per_s"] / HBM_RATE
    res["share_of_f64"] = res["flops_per_s"] / F64_RATE

    def torch_path():
        x = photos.permute(0, 3, 1, 2).float()
        y = F.interpolate(x, size=(s, s), mode="bicubic", antialias=True, align_corners=False)
        if mode == "u8":
            return y.add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return y.clamp_(0, 255).div_(255.0)

    res["torch_ms"], res["torch_all"] = timed(torch_path, steps, warmup)
    got, ref = rs(photos), torch_path()
    if mode == "u8":
        res["torch_max_diff_bytes"] = int((got.to(torch.int16) - ref.to(torch.int16)).abs().max())
    else:
        res["torch_max_diff_of_255"] = float((got - ref).abs().max()) * 255.0
    host = photos.cpu().numpy()
    resample = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]

    def one(a):
        if mode == "u8":
            return np.asarray(Image.fromarray(a, "RGB").resize((s, s), resample))
        return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(a[:, :, c], dtype=np.float32), "F").resize((s, s), resample))
                         for c in range(3)])

    with ThreadPoolExecutor(THREADS) as ex:
        times = []
        for i in range(max(2, min(steps, 3)) + 1):
            t0 = time.perf_counter()
            out = list(ex.map(one, host))
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
    res["pillow_threads"] = THREADS
    res["pillow_ms"] = float(np.median(times))
    want = np.stack(out)
    res["equals_pillow"] = bool(np.array_equal(got.cpu().numpy(), want) if mode == "u8" else
                                np.array_equal(got.cpu().numpy(), np.clip(want, 0, 255).astype(np.float32) / np.float32(255)))
    return res


def run_fid(steps, warmup):
    from PIL import Image
    from wu import fid
    from wu.inception import InceptionV3
    from wu.resample import GPUResampler, read_batches
    n, h, w, bs = 100, 375, 500, 50
    tmp = tempfile.mkdtemp(prefix="bench_resample_")
    for i, a in enumerate(photographs(n, h, w, seed=1).cpu().numpy()):
        Image.fromarray(a, "RGB").save(os.path.join(tmp, f"im{i:03d}.png"), compress_level=1)
    torch.manual_seed(0)
    out = {"config": "fid", "N": n, "h": h, "w": w, "batch": bs, "weights": "random"}
    for rule in ("legacy", "clean"):
        model = InceptionV3(resize=rule).to(DEV)
        for _ in range(max(1, warmup - 1)):
            fid.statistics_of_path(tmp, model, bs, resize=rule)
        times = []
        for _ in range(max(2, steps // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fid.statistics_of_path(tmp, model, bs, resize=rule)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[rule + "_pass_ms"] = float(np.median(times))
        out[rule + "_pass_all"] = [round(t, 1) for t in times]
    batches = list(read_batches(fid.image_files(tmp), bs))
    rs = GPUResampler(299, "bicubic", "f32", "unit")
    out["resampler_ms_per_pass"], _ = timed(lambda: [rs.inception_input(b, s) for b, s in batches], steps, warmup)
    out["resampler_share_of_clean_pass"] = out["resampler_ms_per_pass"] / out["clean_pass_ms"]
    legacy = InceptionV3()
    out["legacy_input_ms_per_pass"], _ = timed(lambda: [legacy.prepare(b) for b, _ in batches], steps, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", nargs="+", default=["flickr", "big_f32", "big_u8", "fid"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs the GPU: no CPU timing is meaningful")
    for name in args.config:
        res = run_fid(args.steps, args.warmup) if name == "fid" else run_config(name, args.steps, args.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
