"""Device time and peak memory of the radial power spectrum (wu.spectrum -> csrc/spectrum.hip) against the composition of the same numbers
out of torch ops on the same GPU: float64 luma, ``torch.fft.rfft2`` (or, where this torch build has no FFT backend, float64 ``matmul``
against the same twiddle tables), ``abs^2``, and a dense one-hot ``matmul`` for the radial bins.

    python scratch/bench_spectrum.py --config split [--steps 5] [--warmup 2]

  split     1000 images of 3 x 224 x 224 uint8 (NHWC views): the test split, 500 + 500
  pggan     8192 images of 3 x 256 x 256 uint8
  s512      64 images of 3 x 512 x 512 uint8
  s1024     16 images of 3 x 1024 x 1024 uint8
  sweep     5 x 16 float32 outputs of 3 x 224 x 224, one row at a time, as ``SpectralDiscrepancy.update`` sees them
  evalshare ``ClassTransferEval.update`` of 16 images at 224 x 224 over 5 classes, with and without ``spectrum=``

One JSON line per config: the medians over the timed calls (device events around one whole call, inputs resident; the two candidates take
turns inside every round), all the times, the peak device memory above the resident inputs, how far the two results lie apart, whether two
fused runs and two chunkings gave the same bytes, and the fused path's workspace.  A fused path slower than the composition is marked LOSS.
One config per process keeps a config's allocator state out of the next one's peak."""
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

CONFIGS = {"split": (1000, 224, "uint8"), "pggan": (8192, 256, "uint8"), "s512": (64, 512, "uint8"), "s1024": (16, 1024, "uint8"),
           "sweep": (80, 224, "float32")}


def timed_alternating(fns, steps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: (round(float(np.median(v)), 3), [round(t, 3) for t in v]) for k, v in times.items()}


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def _images(n, size, kind, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    parts = []
    for i in range(0, n, 256):
        k = min(256, n - i)
        coarse = torch.rand((k, size // 8, size // 8, 3), generator=gen, device=dev)
        x = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2) * 0.6 + 0.4 * torch.rand((k, size, size, 3), generator=gen, device=dev)
        parts.append((x * 255).round().to(torch.uint8) if kind == "uint8" else (x * 2 - 1).permute(0, 3, 1, 2).contiguous())
    x = torch.cat(parts)
    return x.permute(0, 3, 1, 2) if kind == "uint8" else x          # uint8: NHWC storage, read through its strides


def has_fft(dev):
    try:
        torch.fft.rfft2(torch.zeros(2, 6, 10, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return True
    except RuntimeError:
        return False


def make_composition(size, value_range, dev, fft, chunk):
    from wu import paired, spectrum
    scale, shift, L = paired.range_mapping(value_range)
    idx, count, _ = spectrum.radial_bins(size, size)
    K = count.shape[0]
    weight = np.where((np.arange(size // 2 + 1) > 0) & (2 * np.arange(size // 2 + 1) < size), 2.0, 1.0)
    onehot = np.zeros((idx.size, K))
    onehot[np.arange(idx.size), idx.reshape(-1)] = np.broadcast_to(weight, idx.shape).reshape(-1)
    onehot = torch.from_numpy(onehot / count / float(size * size) ** 2).to(dev)
    if not fft:
        c, s = spectrum.twiddles(size)
        k = (np.arange(size)[:, None] * np.arange(size)[None, :]) % size
        C, S = torch.from_numpy(c[k]).to(dev), torch.from_numpy(s[k]).to(dev)          # (size, size) tables: the rival may keep them

    def comp(x):
        out = []
        for i in range(0, x.shape[0], chunk):
            s = (x[i:i + chunk].double() * scale + shift) / L
            y = (0.299 * s[:, 0] + 0.587 * s[:, 1]) + 0.114 * s[:, 2]
            if fft:
                p = torch.fft.rfft2(y)
                p = p.real * p.real + p.imag * p.imag
            else:
                wh = size // 2 + 1
                tr, ti = y @ C[:, :wh], -(y @ S[:, :wh])
                xr, xi = C @ tr + S @ ti, C @ ti - S @ tr
                p = xr * xr + xi * xi
            out.append(p.reshape(p.shape[0], -1) @ onehot)
        return torch.cat(out)
    return comp


def eval_share(a):
    import cunet
    from wu.evaluate import ClassTransferEval, SpectralDiscrepancy
    from wu.train_step import StandInEstimator
    nc, b, size, dev = 5, 16, 224, torch.device("cuda:0")
    torch.manual_seed(0)
    net = cunet.Conditional_UNet(nc, precision="bf16").to(dev).eval()
    cls = StandInEstimator(nc).to(dev).eval()
    batch = (torch.rand((b, 3, size, size)) * 2 - 1).to(dev)
    plain = ClassTransferEval(net, cls, nc)
    with_s = ClassTransferEval(net, cls, nc, spectrum=SpectralDiscrepancy())
    fakes = net.sweep(batch, torch.eye(nc, device=dev), plain.max_images)
    times = timed_alternating({"update": lambda: plain.update(batch), "update_with_spectrum": lambda: with_s.update(batch),
                               "spectrum_update_alone": lambda: with_s.spectrum.update(batch, fakes)}, a.steps, a.warmup)
    out = {"config": "evalshare", "classes": nc, "B": b, "size": size, "fakes_dtype": str(fakes.dtype), "steps": a.steps, "warmup": a.warmup}
    for k, (ms, all_ms) in times.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_all"] = ms, all_ms
    out["share_of_update_with_spectrum"] = round((times["update_with_spectrum"][0] - times["update"][0]) / times["update_with_spectrum"][0], 4)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS) + ["evalshare"], required=True)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.config == "evalshare":
        return eval_share(a)
    from wu import _lib, spectrum
    n, size, kind = CONFIGS[a.config]
    dev = torch.device("cuda:0")
    value_range = "uint8" if kind == "uint8" else (-1, 1)
    x = _images(n, size, kind, dev)
    fft = has_fft(dev)
    chunk = spectrum.default_max_images(size, size)
    comp = make_composition(size, value_range, dev, fft, min(n, chunk))
    if a.config == "sweep":
        rows = x.view(5, 16, 3, size, size)

        def fused():
            return torch.stack([spectrum.profiles(r, value_range) for r in rows])

        def rival():
            return torch.stack([comp(r) for r in rows])
    else:
        def fused():
            return spectrum.profiles(x, value_range)

        def rival():
            return comp(x)

    ref = fused()
    again = fused()
    small = (spectrum.profiles(x[:16], value_range, max_images=3), spectrum.profiles(x[:16], value_range, max_images=16))
    got = rival()
    band = slice(1, size // 2 + 1)
    out = {"config": a.config, "images": n, "size": size, "dtype": kind, "steps": a.steps, "warmup": a.warmup,
           "rival": "torch.fft.rfft2" if fft else "float64 matmul against the twiddle tables", "K": int(ref.shape[-1]),
           "max_images_default": chunk, "fused_workspace_bytes": int(_lib.load().wu_spectrum_workspace_bytes(min(n, chunk), size, size)),
           "max_rel_diff_bins_1_to_nyquist": float(((got - ref).abs() / ref)[..., band].max()),
           "same_bits_two_runs": bool(torch.equal(ref, again)), "same_bits_two_chunkings": bool(torch.equal(*small))}
    del got, again, small
    times = timed_alternating({"fused": fused, "torch": rival}, a.steps, a.warmup)
    for k, (ms, all_ms) in times.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_all"] = ms, all_ms
    out["fused_vs_torch"] = ("LOSS " if times["fused"][0] > times["torch"][0] else "") + f"{times['torch'][0] / times['fused'][0]:.2f}x"
    out["fused_peak_extra_bytes"], out["torch_peak_extra_bytes"] = peak_extra(fused), peak_extra(rival)
    flops = n * (2.0 * size * size * 2 * (size // 2 + 1) + 2.0 * 2 * size * size * 2 * (size // 2 + 1))
    out["fused_fp64_tflops"] = round(flops / times["fused"][0] / 1e9, 2)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
