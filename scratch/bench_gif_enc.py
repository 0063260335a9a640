"""GIF benchmark: wu.infer_driver.save_demo(frames, "x.gif") with wu.gif_enc.GPUGifEncoder (csrc/gif_enc.hip) against the same call without
it -- Pillow's quantiser and LZW on the host over the frames fetched as raw RGB, the path of the parent commit -- on one MI355X.

    python scratch/bench_gif_enc.py [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o gif -- python scratch/bench_gif_enc.py --mode device      # kernel rows, run of its own
    python scratch/bench_gif_enc.py --mode quality [--paths default,best]        # the quality options against the defaults, same call
    WU_AB_LIB=scratch/_oldlib/libwu_old.so python scratch/bench_gif_enc.py --mode quality --paths default     # the defaults on another build

--mode quality: ``encode`` (launch + fetch, the file as bytes; nothing written) of the demo table with the default encoder and with
``GPUGifEncoder.best()``, one warm-up call each, then `--runs` calls each, alternating, device events around the whole call and a
synchronise behind it; median (min .. max) and the file sizes.  --mode device takes --paths too, for the kernel rows of both.

Shapes: the grid bench's demo table (B=16, nc=5, 256^2, T=8 frames, 14 entries in ping-pong order) and B=4 at 224^2, T=10.  The sources are
smooth random fields with a little noise on top (bilinear upsampling of 8x8 noise plus 2 % white noise) rather than white noise, which no
demo shows; the frames keep the tables' padding, so one frame also measures the histogram's flat case.
Method: one warm-up call per path, then `--runs` calls per path, alternating, each timed on the wall clock (the call ends with the file on
disk) and with time.process_time (host CPU seconds of the process, all threads); median (min .. max).  Bytes over the link: the Pillow path
fetches T H W 3 bytes; the encoder's path fetches the T byte counts and the blocks (its own stats).  Results go to profiles/gif_enc_bench.md
by hand, with the command line.
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


def spread(v, unit=1e3):
    return f"{statistics.median(v) * unit:.1f} ({min(v) * unit:.1f} .. {max(v) * unit:.1f})"


def smooth(shape, g, dev):
    """Values in [-1, 1]: low-frequency fields, a little noise."""
    lead, (h, w) = shape[:-2], shape[-2:]
    n = 1
    for d in lead:
        n *= d
    low = torch.rand(n, 1, 8, 8, generator=g).to(dev)
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False).view(*lead, h, w)
    return (x * 2 - 1 + 0.02 * torch.randn(*shape, generator=g).to(dev)).clamp(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "device", "quality"])
    ap.add_argument("--paths", default="default", help="--mode quality / device: comma-separated, of default, nearest, ordered, exact, global, best")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wu import grid
    from wu import infer_driver as D
    from wu.gif_enc import GPUGifEncoder, ping_pong

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"cmd": " ".join(sys.argv), "gpu": torch.cuda.get_device_name(0), "runs": a.runs}
    enc = GPUGifEncoder(dev)
    options = {"default": {}, "nearest": dict(mapping="nearest"), "ordered": dict(mapping="nearest", dither="ordered"), "exact": dict(exact=True),
               "global": dict(palette="global"), "best": dict(mapping="nearest", dither="ordered", exact=True, palette="global")}
    paths = {k: (enc if k == "default" else GPUGifEncoder(dev, **options[k])) for k in a.paths.split(",")}
    for name, (T, nc, B, S) in {"demo_B16_nc5_256_T8": (8, 5, 16, 256), "demo_B4_nc5_224_T10": (10, 5, 4, 224)}.items():
        batch = smooth((B, 3, S, S), g, dev)
        results = smooth((T, nc, B, 3, S, S), g, dev)
        frames = grid.demo_tables(batch, results)
        torch.cuda.synchronize()
        row = {"frames": list(frames.shape), "entries": len(ping_pong(T))}
        if a.mode == "device":
            for e in paths.values():
                for _ in range(5):
                    e.encode(frames, 1000 // T, 0, ping_pong(T))
            torch.cuda.synchronize()
            res[name] = row
            continue
        if a.mode == "quality":
            ms, size = {k: [] for k in paths}, {}
            for k, e in paths.items():
                size[k] = len(e.encode(frames, 1000 // T, 0, ping_pong(T)))
            for r in range(a.runs):                                          # alternate the paths
                for k in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    paths[k].encode(frames, 1000 // T, 0, ping_pong(T))
                    e1.record()
                    torch.cuda.synchronize()
                    ms[k].append(e0.elapsed_time(e1) * 1e-3)
            for k in paths:
                row[k + "_call_ms"] = spread(ms[k])
                row[k + "_file_bytes"] = size[k]
            res[name] = row
            print(name, json.dumps(row), flush=True)
            continue
        with tempfile.TemporaryDirectory() as tmp:
            paths = {"gpu": os.path.join(tmp, "gpu.gif"), "pillow": os.path.join(tmp, "pillow.gif")}
            calls = {"gpu": lambda: D.save_demo(frames, paths["gpu"], gif_encoder=enc), "pillow": lambda: D.save_demo(frames, paths["pillow"])}
            for fn in calls.values():
                fn()
            wall, cpu = {k: [] for k in calls}, {k: [] for k in calls}
            for r in range(a.runs):                                          # alternate the two paths
                for k in (("gpu", "pillow") if r % 2 == 0 else ("pillow", "gpu")):
                    torch.cuda.synchronize()
                    c0, t0 = time.process_time(), time.perf_counter()
                    calls[k]()
                    wall[k].append(time.perf_counter() - t0)
                    cpu[k].append(time.process_time() - c0)
            before = enc.stats["bytes"]
            calls["gpu"]()
            row.update({
                "gpu_wall_ms": spread(wall["gpu"]), "pillow_wall_ms": spread(wall["pillow"]),
                "gpu_host_cpu_ms": spread(cpu["gpu"]), "pillow_host_cpu_ms": spread(cpu["pillow"]),
                "gpu_link_bytes": enc.stats["bytes"] - before + 4 * T, "pillow_link_bytes": frames.numel(),
                "gpu_file_bytes": os.path.getsize(paths["gpu"]), "pillow_file_bytes": os.path.getsize(paths["pillow"]),
                "wall_ratio_of_medians": round(statistics.median(wall["pillow"]) / statistics.median(wall["gpu"]), 2),
                "gpu_clears_bar": bool(max(wall["gpu"]) < min(wall["pillow"])),
            })
            from PIL import Image
            im = Image.open(paths["gpu"])
            row["gpu_file_frames_in_pillow"] = im.n_frames
        res[name] = row
        print(name, json.dumps(row), flush=True)
    enc.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
