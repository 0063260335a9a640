"""PNG decode benchmark: wu.png.GPUPngDecoder against the path it replaces -- Pillow's Image.open(...).convert("RGB") per file, stacked
and copied to the GPU, as wu.fid reads a directory -- on the same machine, the same files, and next to it Pillow on a 16-thread pool.

    python scratch/bench_png_dec.py                       # host comparison: images per second, and the two launches timed by events
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o png_dec -- python scratch/bench_png_dec.py --mode device       # kernel times, run of its own

Workload: the sweep's own files -- images with natural statistics tiled from the decoded fixtures to 512^2 (the sweep's size) and 224^2,
written by wu.png_enc.GPUPngEncoder (literal-only dynamic blocks, 25 and 5 segments per image); batches of 16 and 64; the files are
bytes in memory, so no disk is measured.  Warm-up, then 5 runs per path of at least 0.5 s each (whole passes over the files), the paths
alternating (order swapped every run); median (min .. max) reported.  All paths return the same pixels (checked outside the timing).
Results go to profiles/png_dec_bench.md by hand, with the command line.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_jpeg_enc import cpu_model, natural_images, spread          # noqa: E402  (also puts weather-unet_amd on the path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="host", choices=["host", "device"])
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="a run makes whole passes over the files until it has lasted this long")
    a = ap.parse_args()
    import PIL
    from PIL import Image, features
    from wu import _lib
    from wu.layout import stream_ptr
    from wu.png import GPUPngDecoder
    from wu.png_enc import GPUPngEncoder

    threads = min(16, a.threads)
    dev = torch.device("cuda:0")
    res = {"cmd": " ".join(sys.argv), "pillow_version": PIL.__version__, "zlib": features.version("zlib"), "cpu": cpu_model(),
           "threads": threads, "images": a.images, "gpu": torch.cuda.get_device_name(0)}
    pool = ThreadPoolExecutor(max_workers=threads)
    enc = GPUPngEncoder(dev, threads=threads)
    dec = GPUPngDecoder(dev, threads=threads)

    def pillow_one(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)

    def pillow_serial(files):                             # wu.fid.statistics_of_path without a switch
        return torch.from_numpy(np.stack([pillow_one(f) for f in files])).to(dev)

    def pillow_pool(files):
        return torch.from_numpy(np.stack(list(pool.map(pillow_one, files)))).to(dev)

    def native(files):
        return dec.decode_batch(files)[0]

    shapes = [(224, 16), (224, 64), (512, 16), (512, 64)] if a.mode == "host" else [(512, 16)]
    for size, batch in shapes:
        n_img = a.images if a.mode == "host" else batch
        imgs = torch.from_numpy(natural_images(n_img, size)).to(dev)
        files = []
        for i in range(0, n_img, batch):
            files.append(enc.encode_batch(imgs[i:i + batch]))
        key = f"{size}x{size}_b{batch}"
        got = native(files[0])
        assert torch.equal(got, imgs[:batch]) and torch.equal(pillow_serial(files[0]), got)      # the same pixels
        assert dec.stats["fallback"] == 0
        hb = dec.prepare(files[0])
        s = dec.buffer_sizes(hb)
        buf = hb.staging.tensor[:hb.used].to(dev)
        ws = torch.empty(s["workspace"], dtype=torch.uint8, device=dev)
        out = torch.empty((hb.n, hb.hmax, hb.wmax, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(hb.n, dtype=torch.int32, device=dev)
        base = buf.data_ptr()

        def launches():
            _lib.call("wu_png_dec_decode", base, s["source"], base + hb.off["desc"], s["desc"], base + hb.off["seg"], s["seg"], hb.n_segments,
                      ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), status.data_ptr(), status.numel() * 4, hb.n, hb.hmax, hb.wmax,
                      stream_ptr())

        if a.mode == "device":
            for _ in range(10):
                launches()
            torch.cuda.synchronize()
            res[key] = {"launches": 11, "segments": hb.n_segments}
            hb.release()
            continue
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t = []
        for _ in range(12):
            ev[0].record()
            launches()
            ev[1].record()
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]) * 1e3)
        assert torch.equal(out, got) and not status.any()
        hb.release()
        paths = (("pillow_serial", pillow_serial), ("pillow_pool", pillow_pool), ("native", native))
        for _, fn in paths:
            for b in files[:2]:
                fn(b)
        runs = {name: [] for name, _ in paths}
        for r in range(a.runs):
            for name, fn in paths if r % 2 == 0 else paths[::-1]:
                w0, c0 = time.perf_counter(), time.process_time()
                n = 0
                while n == 0 or time.perf_counter() - w0 < a.min_seconds:
                    for b in files:
                        fn(b)
                        n += len(b)
                torch.cuda.synchronize()
                runs[name].append({"images_per_s": n / (time.perf_counter() - w0), "cpu_ms_per_image": 1e3 * (time.process_time() - c0) / n})
        res[key] = {name: {k: spread([v[k] for v in runs[name]]) for k in ("images_per_s", "cpu_ms_per_image")} for name in runs}
        res[key]["segments_per_batch"] = hb.n_segments
        res[key]["file_bytes_per_image"] = sum(map(len, files[0])) / len(files[0])
        res[key]["two_launches_us_events"] = spread(t[2:])

    enc.close()
    dec.close()
    pool.shutdown()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
