"""JPEG decode benchmark: wu.jpeg.GPUJpegDecoder against the Pillow path on the same machine, same bytes, same threads.

    python scratch/bench_jpeg.py                      # host comparison + host breakdown + device timing (events) + end-to-end line
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o jpeg -- python scratch/bench_jpeg.py --mode device      # kernel times of ONE batch, run of its own
    python scratch/bench_jpeg.py --mode progressive   # the same pixels saved with progressive=True: Pillow, the default decoder (every
                                                      # file takes its Pillow fallback) and coverage="extended" (native), alternating

Workload: 512 generated photo-like JPEGs, 500x375 and 375x500 mixed, quality 85, 4:2:0, held in memory as bytes (no disk in the
timing); batches of 64; 16 host threads on both sides; warm-up, then >= 20 batches per run, 5 runs, the two paths alternating inside
one process; median and spread (min .. max) reported.  Results go to profiles/jpeg_bench.md by hand, with the command line.
"""
import argparse
import io
import json
import os
import platform
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "weather-unet_amd"))


def photo_like(h, w, seed):
    """Smooth large-scale structure, a few edges, sensor-like noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([120 + 80 * np.sin(xx / (37.0 + seed % 11) + seed) * np.cos(yy / 53.0), 110 + 70 * np.cos((xx + yy) / 61.0 + seed),
                    90 + 60 * np.sin(yy / (29.0 + seed % 7))], -1)
    for _ in range(6):                                                  # rectangles: hard edges
        y0, x0 = rng.integers(0, h - 20), rng.integers(0, w - 20)
        img[y0:y0 + rng.integers(10, h // 2), x0:x0 + rng.integers(10, w // 2)] += rng.normal(0, 40, 3)
    return np.clip(img + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def make_files(n, progressive=False):
    from PIL import Image
    out = []
    for k in range(n):
        h, w = (375, 500) if k % 2 == 0 else (500, 375)
        f = io.BytesIO()
        Image.fromarray(photo_like(h, w, k)).save(f, "JPEG", quality=85, subsampling=2, **(dict(progressive=True) if progressive else {}))
        out.append(f.getvalue())
    return out


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


def algorithm_bytes(infos, hmax, wmax):
    """Bytes the two-stage algorithm has to move for one batch, from shapes: coefficients read once (2 B each), the uint8 planes
    written and read once, RGB written once at 3 B per pixel of the PADDED batch."""
    blocks = sum(i.total_blocks for i in infos)
    return {"coef": blocks * 128, "planes_rw": 2 * blocks * 64, "rgb": len(infos) * hmax * wmax * 3,
            "total": blocks * 128 + 2 * blocks * 64 + len(infos) * hmax * wmax * 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "host", "device", "e2e", "progressive"])
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3, help="passes over the files per run (3 x 8 = 24 batches of 64)")
    a = ap.parse_args()
    import PIL
    from PIL import Image, features
    from wu import jpeg
    from wu.jpeg import GPUJpegDecoder

    threads = min(16, a.threads)
    res = {"cmd": " ".join(sys.argv), "pillow_version": PIL.__version__, "libjpeg": features.version("jpg"), "libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")),
           "cpu": cpu_model(), "threads": threads, "files": a.files, "batch": a.batch, "gpu": torch.cuda.get_device_name(0)}
    files = make_files(a.files, progressive=a.mode == "progressive")
    res["mean_file_bytes"] = sum(map(len, files)) / len(files)
    batches = [files[i:i + a.batch] for i in range(0, len(files), a.batch)]
    dev = torch.device("cuda:0")
    dec = GPUJpegDecoder(dev, threads=threads)
    pool = ThreadPoolExecutor(max_workers=threads)

    def pillow_one(b):
        return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))

    def pillow_batch(items):
        arrs = list(pool.map(pillow_one, items))
        hmax, wmax = max(x.shape[0] for x in arrs), max(x.shape[1] for x in arrs)
        buf = np.zeros((len(arrs), hmax, wmax, 3), dtype=np.uint8)
        for i, x in enumerate(arrs):
            buf[i, :x.shape[0], :x.shape[1]] = x
        t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        return t

    def native_batch(items):
        t, _ = dec.decode_batch(items)
        torch.cuda.synchronize()
        return t

    # the two paths produce the same tensor (checked once, outside the timing)
    assert torch.equal(pillow_batch(batches[0]), native_batch(batches[0]))
    assert dec.stats["fallback"] == (len(batches[0]) if a.mode == "progressive" else 0)

    if a.mode == "progressive":
        # The progressive copy of the set.  "fallback": the default decoder, where every file is refused ("progressive") and decoded by
        # Pillow on the worker thread -- what a revision without the extended coverage does with these files; "extended": the scans run
        # natively on the worker threads.  A library without wu_jpeg_parse_ex measures the first two only.
        paths = [("pillow", pillow_batch), ("fallback", native_batch)]
        ext = None
        if hasattr(jpeg, "COVERAGE"):
            ext = GPUJpegDecoder(dev, threads=threads, coverage="extended")

            def extended_batch(items):
                t, _ = ext.decode_batch(items)
                torch.cuda.synchronize()
                return t
            assert torch.equal(pillow_batch(batches[0]), extended_batch(batches[0])) and ext.stats["fallback"] == 0
            paths.append(("extended", extended_batch))
        for _, fn in paths:
            for b in batches[:3]:
                fn(b)
        runs = {name: [] for name, _ in paths}
        for r in range(a.runs):
            for name, fn in paths[r % len(paths):] + paths[:r % len(paths)]:
                w0, c0 = time.perf_counter(), time.process_time()
                n = 0
                for _ in range(a.passes):
                    for b in batches:
                        fn(b)
                        n += len(b)
                runs[name].append({"images_per_s": n / (time.perf_counter() - w0), "cpu_s_per_image": (time.process_time() - c0) / n})
        res["progressive"] = {name: {k: spread([x[k] for x in runs[name]]) for k in ("images_per_s", "cpu_s_per_image")} for name in runs}
        res["progressive"]["batches_per_run"] = a.passes * len(batches)
        if ext is not None:                                              # one thread: the scans of one file against Pillow's decode of it
            lib = jpeg._lib.load()
            coef = np.empty(8 << 20, dtype=np.int16)
            q = np.empty((3, 64), dtype=np.uint16)
            t0 = time.perf_counter()
            for b in files[:128]:
                info = jpeg._parse_bytes(lib, b, jpeg.COVERAGE["extended"])
                jpeg._entropy_into(lib, b, info, coef.ctypes.data, coef.nbytes, q.ctypes.data)
            t1 = time.perf_counter()
            for b in files[:128]:
                pillow_one(b)
            res["progressive"]["single_thread_s_per_image"] = {"parse_and_all_scans": (t1 - t0) / 128, "pillow_decode": (time.perf_counter() - t1) / 128}
            ext.close()

    if a.mode in ("all", "host"):
        for fn in (pillow_batch, native_batch):                         # warm-up: thread pools, pinned staging, allocator
            for b in batches[:3]:
                fn(b)
        runs = {"pillow": [], "native": []}
        for r in range(a.runs):
            for name, fn in (("pillow", pillow_batch), ("native", native_batch)) if r % 2 == 0 else (("native", native_batch), ("pillow", pillow_batch)):
                w0, c0 = time.perf_counter(), time.process_time()
                n = 0
                for _ in range(a.passes):
                    for b in batches:
                        fn(b)
                        n += len(b)
                runs[name].append({"images_per_s": n / (time.perf_counter() - w0), "cpu_s_per_image": (time.process_time() - c0) / n})
        for name in runs:
            res[name] = {k: spread([x[k] for x in runs[name]]) for k in ("images_per_s", "cpu_s_per_image")}
            res[name]["batches_per_run"] = a.passes * len(batches)
        # where the host time of the native path goes: one thread, time.perf_counter around the calls
        lib = jpeg._lib.load()
        t_parse = t_huff = 0.0
        coef = np.empty(8 << 20, dtype=np.int16)
        q = np.empty((3, 64), dtype=np.uint16)
        for b in files[:128]:
            t0 = time.perf_counter()
            info = jpeg._parse_bytes(lib, b)
            t1 = time.perf_counter()
            jpeg._entropy_into(lib, b, info, coef.ctypes.data, coef.nbytes, q.ctypes.data)
            t2 = time.perf_counter()
            t_parse += t1 - t0
            t_huff += t2 - t1
        t0 = time.perf_counter()
        for b in batches[:2]:
            dec.prepare(b).release()
        t_prep = (time.perf_counter() - t0) / (2 * a.batch)
        t0 = time.perf_counter()
        for b in files[:128]:
            pillow_one(b)
        res["host_breakdown_single_thread_s_per_image"] = {"parse": t_parse / 128, "huffman_incl_zero_fill_into_staging": t_huff / 128,
                                                           "prepare_wall_per_image_16_threads": t_prep,
                                                           "pillow_decode": (time.perf_counter() - t0) / 128,
                                                           "staging_copy": 0.0}      # the Huffman stage writes into the staging buffer itself

    if a.mode in ("all", "device"):
        b = batches[0]
        hb = dec.prepare(b)
        infos = [jpeg.parse(x) for x in b]
        by = algorithm_bytes(infos, hb.hmax, hb.wmax)
        res["algorithm_bytes_per_batch"] = by
        res["staged_bytes_per_batch"] = hb.used
        for _ in range(3):
            dec.finish(hb)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_h2d, t_rec = [], []
        for _ in range(10):
            ev[0].record()
            db = dec.upload(hb)
            ev[1].record()
            dec.reconstruct(db)
            ev[2].record()
            torch.cuda.synchronize()
            t_h2d.append(ev[0].elapsed_time(ev[1]))
            t_rec.append(ev[1].elapsed_time(ev[2]))
        res["device_events_ms"] = {"h2d_coefficients_and_descriptors": spread(t_h2d), "reconstruct_two_launches": spread(t_rec)}
        res["reconstruct_bytes_per_s_median"] = by["total"] / (statistics.median(t_rec) * 1e-3)
        rgb = torch.empty((len(b), hb.hmax, hb.wmax, 3), dtype=torch.uint8).pin_memory()
        t_rgb = []
        for _ in range(10):
            ev[0].record()
            rgb.to(dev, non_blocking=True)
            ev[1].record()
            torch.cuda.synchronize()
            t_rgb.append(ev[0].elapsed_time(ev[1]))
        res["device_events_ms"]["h2d_of_an_rgb_batch_same_shape_pinned"] = spread(t_rgb)
        hb.release()

    if a.mode in ("all", "e2e"):
        from wu.data import JpegBatchLoader
        from wu.input_pipeline import GPUInputPipeline
        from wu.train_step import WeatherTransferStep
        B, S, iters = 32, 224, 48
        gan = WeatherTransferStep(5, mode="cls", precision="bf16", device=dev, seed=0)
        pipe = GPUInputPipeline(S, augmentation=True, seed=0)
        g = torch.Generator().manual_seed(0)
        x = (torch.rand((B, 3, S, S), generator=g) * 2 - 1).to(dev)
        xr = (torch.rand((B, 3, S, S), generator=g) * 2 - 1).to(dev)
        many = (files * (1 + (2 * B * iters) // len(files)))[:2 * B * iters]

        def resident():
            for _ in range(iters):
                gan.step(x, xr)
            torch.cuda.synchronize()

        def loaded():
            ld = JpegBatchLoader(many, batch_size=2 * B, pipeline=pipe, decoder=dec, prefetch=2)      # one batch = images + rand_images
            for images, _, _ in ld:
                gan.step(images[:B], images[B:])
            torch.cuda.synchronize()

        src_u8, src_sizes = dec.decode_batch(many[:2 * B])

        def resident_u8():                                              # decoded uint8 batch resident, transforms per iteration: isolates the decoder's share
            for _ in range(iters):
                images = pipe(src_u8, src_sizes)
                gan.step(images[:B], images[B:])
            torch.cuda.synchronize()

        order = [("resident", resident), ("resident_u8_plus_pipeline", resident_u8), ("loader", loaded)]
        for _, fn in order:
            fn()
        rates = {name: [] for name, _ in order}
        for r in range(a.runs):
            for name, fn in order if r % 2 == 0 else order[::-1]:
                t0 = time.perf_counter()
                fn()
                rates[name].append(iters / (time.perf_counter() - t0))
        res["e2e_gan_cls_b32_224_standin_iters_per_s"] = {k: spread(v) for k, v in rates.items()}
        res["e2e_ratio_loader_over_resident"] = statistics.median(rates["loader"]) / statistics.median(rates["resident"])

    dec.close()
    pool.shutdown()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
