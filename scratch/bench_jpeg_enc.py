"""JPEG encode benchmark: wu.jpeg_enc.GPUJpegEncoder against the path users had before it -- to_uint8(...).cpu() and Pillow's Image.save
into memory on a 16-thread pool -- on the same machine, same pixels, same threads.

    python scratch/bench_jpeg_enc.py                      # host comparison (4 shapes) + end-to-end class sweep to a tmpfs directory
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o jpeg_enc -- python scratch/bench_jpeg_enc.py --mode device      # kernel times, run of its own

Workload: 256 images with natural statistics -- the repository's JPEG / PNG fixtures decoded, resized and tiled to 224^2 and 512^2 with
varying scale, offset and flip -- resident on the GPU as an (N, 3, S, S) fp32 batch in [0, 1] (what normalize_minmax leaves); batches of
16 and 64; warm-up, then 5 runs per path of at least 0.5 s each (whole passes over the 256 images), the two paths alternating (order
swapped every run); median (min .. max) reported.  Results go to profiles/jpeg_enc_bench.md by hand, with the command line.
"""
import argparse
import glob
import io
import json
import os
import platform
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "weather-unet_amd"))


def natural_images(n, size):
    """n (size, size, 3) uint8 images tiled from the decoded fixtures."""
    from PIL import Image
    srcs = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*"))):
        if p.endswith((".jpg", ".png")):
            try:
                srcs.append(Image.open(p).convert("RGB").copy())
            except Exception:          # noqa: BLE001 -- the deliberately truncated fixture
                pass
    assert srcs
    rng = np.random.default_rng(0)
    out = []
    for k in range(n):
        im = srcs[k % len(srcs)]
        scale = size / max(im.size) * rng.uniform(0.6, 1.6)
        im = im.resize((max(8, int(im.size[0] * scale)), max(8, int(im.size[1] * scale))), Image.BICUBIC)
        a = np.asarray(im)
        if rng.random() < 0.5:
            a = a[:, ::-1]
        reps = (-(-2 * size // a.shape[0]), -(-2 * size // a.shape[1]), 1)
        t = np.tile(np.concatenate([a, a[::-1]], 0), reps)
        y0, x0 = rng.integers(0, t.shape[0] - size), rng.integers(0, t.shape[1] - size)
        out.append(np.ascontiguousarray(t[y0:y0 + size, x0:x0 + size]))
    return np.stack(out)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor()


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "host", "device", "e2e"])
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="a run makes whole passes over the images until it has lasted this long")
    a = ap.parse_args()
    import PIL
    from PIL import Image, features
    from wu.infer_driver import class_sweep_to_dir, normalize_minmax, signal_sweep, to_uint8
    from wu.jpeg_enc import GPUJpegEncoder

    threads = min(16, a.threads)
    dev = torch.device("cuda:0")
    res = {"cmd": " ".join(sys.argv), "pillow_version": PIL.__version__, "libjpeg": features.version("jpg"),
           "libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")), "cpu": cpu_model(), "threads": threads, "images": a.images,
           "gpu": torch.cuda.get_device_name(0)}
    pool = ThreadPoolExecutor(max_workers=threads)
    enc = GPUJpegEncoder(dev, threads=threads)

    def pillow_one(rgb):
        f = io.BytesIO()
        Image.fromarray(rgb).save(f, "JPEG")
        return f.getvalue()

    def pillow_batch(x):
        return list(pool.map(pillow_one, to_uint8(x).cpu().numpy()))

    def native_batch(x):
        return enc.encode_batch(x)

    if a.mode in ("all", "host", "device"):
        shapes = [(224, 16), (224, 64), (512, 16), (512, 64)] if a.mode != "device" else [(512, 16)]
        for size, batch in shapes:
            imgs = natural_images(a.images if a.mode != "device" else batch, size)
            x = (torch.from_numpy(imgs).to(dev).permute(0, 3, 1, 2).float() / 255).contiguous()
            batches = [x[i:i + batch] for i in range(0, x.shape[0], batch)]
            ref, got = pillow_batch(batches[0]), native_batch(batches[0])             # same files, checked outside the timing
            assert ref == got and enc.stats["fallback"] == 0
            key = f"{size}x{size}_b{batch}"
            if a.mode == "device":
                for _ in range(10):
                    enc.launch(batches[0])
                torch.cuda.synchronize()
                res[key] = {"launches": 11}             # the equality check above + these 10
                continue
            for fn in (pillow_batch, native_batch):
                for b in batches[:2]:
                    fn(b)
            runs = {"pillow": [], "native": []}
            nbytes = nfiles = 0
            for r in range(a.runs):
                order = (("pillow", pillow_batch), ("native", native_batch))
                for name, fn in order if r % 2 == 0 else order[::-1]:
                    w0, c0 = time.perf_counter(), time.process_time()
                    n = 0
                    while n == 0 or time.perf_counter() - w0 < a.min_seconds:      # whole passes; a run of a few ms would measure one hiccup
                        for b in batches:
                            files = fn(b)
                            n += len(files)
                            if name == "native":
                                nbytes += sum(map(len, files))
                                nfiles += len(files)
                    runs[name].append({"images_per_s": n / (time.perf_counter() - w0), "cpu_ms_per_image": 1e3 * (time.process_time() - c0) / n})
            res[key] = {name: {k: spread([v[k] for v in runs[name]]) for k in ("images_per_s", "cpu_ms_per_image")} for name in runs}
            res[key]["d2h_bytes_per_image"] = {"pillow": size * size * 3, "native": nbytes / nfiles + 8}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            t = []
            for _ in range(10):
                ev[0].record()
                enc.launch(batches[0])
                ev[1].record()
                torch.cuda.synchronize()
                t.append(ev[0].elapsed_time(ev[1]) * 1e3)
            res[key]["launch_five_kernels_us_events"] = spread(t)
        assert enc.stats["fallback"] == 0

    if a.mode in ("all", "e2e"):
        import cunet
        from wu.graph_infer import GraphedUNet
        B, S, nc, iters = 16, 512, 5, 4
        torch.manual_seed(0)
        net = cunet.Conditional_UNet(nc, precision="bf16").to(dev).eval()
        graphed = GraphedUNet(net, B, S)
        batch = (torch.from_numpy(natural_images(B, S)).to(dev).permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
        names = [f"class{i}" for i in range(nc)]
        stems = [f"img{j:04d}" for j in range(B)]
        labels = [j % nc for j in range(B)]
        tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)

        def with_encoder():
            class_sweep_to_dir(net, batch, stems, labels, names, tmp, graphed=graphed, encoder=enc)

        def save_one(arg):
            Image.fromarray(arg[0]).save(arg[1])

        def with_pillow():                                             # the same loop with the writer users had: to_uint8().cpu() + Image.save on the pool
            rows = torch.eye(nc, device=dev)
            for i in range(nc):
                out = signal_sweep(net, batch, rows[i:i + 1], True, graphed)[0]
                rgb = to_uint8(out).cpu().numpy()
                list(pool.map(save_one, [(rgb[j], os.path.join(tmp, f"{names[labels[j]]}_{stems[j]}_{names[i]}.jpg")) for j in range(B)]))

        def forward_only():
            rows = torch.eye(nc, device=dev)
            for i in range(nc):
                normalize_minmax(signal_sweep(net, batch, rows[i:i + 1], False, graphed)[0])
            torch.cuda.synchronize()

        order = [("forward_only", forward_only), ("pillow_writer", with_pillow), ("gpu_encoder", with_encoder)]
        for _, fn in order:
            fn()
        rates = {name: [] for name, _ in order}
        for r in range(a.runs):
            for name, fn in order if r % 2 == 0 else order[::-1]:
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                rates[name].append(iters / (time.perf_counter() - t0))
        res["e2e_class_sweep_512_b16_graph_sweeps_per_s"] = {k: spread(v) for k, v in rates.items()}
        res["e2e_images_per_sweep"] = nc * B
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)

    enc.close()
    pool.shutdown()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
