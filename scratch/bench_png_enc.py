"""PNG encode benchmark: wu.png_enc.GPUPngEncoder against the path users have without it -- to_uint8(...).cpu() and Pillow's Image.save
(PNG, Pillow's defaults) into memory on a 16-thread pool -- on the same machine, same pixels, same threads.

    python scratch/bench_png_enc.py                       # host comparison (4 shapes) + end-to-end class sweep to a tmpfs directory
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o png_enc -- python scratch/bench_png_enc.py --mode device       # kernel times, run of its own
    python scratch/bench_png_enc.py --mode ab --matching lz77     # device times of one launch chain: parent library (if built), literal-only, LZ77

``--matching lz77`` runs every mode with ``GPUPngEncoder(matching="lz77")``.  ``--mode ab``: on two batches -- the 512^2 batch of 16 natural
images of ``--mode device`` and a grid-like batch (8 demo tables of 1 + 5 columns and 4 rows of 256^2 cells, input column repeated, 2 px
padding) -- the time between two events around ONE launch chain, 21 times per path, parent and literal-only alternating, then LZ77; median
(min .. max).  Paths:
``parent`` = wu_png_enc_encode of scratch/_oldlib/libwu_old.so (scratch/build_baseline_lib.sh; skipped if absent), ``none`` = this tree's
literal-only chain (``none_again``: the same once more, for the spread between two identical paths), ``lz77`` = this tree's chain with
matching.  File bytes per path beside the times.

Workload: bench_jpeg_enc.py's -- images with natural statistics tiled from the decoded fixtures to 224^2 and 512^2, resident on the GPU
as an (N, 3, S, S) fp32 batch in [0, 1]; batches of 16 and 64; warm-up, then 5 runs per path of at least 0.5 s each (whole passes over
the images), the two paths alternating (order swapped every run); median (min .. max) reported.  The files differ (no LZ77 matching on
the GPU), so the size ratio is reported next to the rates, and both decode to the same pixels (checked outside the timing).  Results go
to profiles/png_enc_bench.md by hand, with the command line.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_jpeg_enc import cpu_model, natural_images, spread          # noqa: E402  (also puts weather-unet_amd on the path)


def demo_table_batch(frames, rows, cols, cell):
    """(frames, Hg, Wg, 3) uint8 tables: ``rows`` x ``cols`` cells of natural images, the first column repeated as the last, 2 px black
    padding -- what save_demo / save_grid hand to the encoder."""
    pad = 2
    imgs = natural_images(frames * rows * (cols - 1), cell)
    out = np.zeros((frames, rows * (cell + pad) + pad, cols * (cell + pad) + pad, 3), np.uint8)
    k = 0
    for f in range(frames):
        for r in range(rows):
            first = None
            for c in range(cols):
                if c < cols - 1:
                    src = imgs[k]
                    k += 1
                    first = src if first is None else first
                else:
                    src = first
                y, x = pad + r * (cell + pad), pad + c * (cell + pad)
                out[f, y:y + cell, x:x + cell] = src
    return out


def ab(dev, threads):
    """Device time of one launch chain per path, and the file sizes."""
    import ctypes
    from wu import _lib
    from wu.layout import stream_ptr
    from wu.png_enc import GPUPngEncoder
    old_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_oldlib", "libwu_old.so")
    old = None
    if os.path.exists(old_path):
        old = ctypes.CDLL(old_path)
        old.wu_png_enc_encode.restype, old.wu_png_enc_encode.argtypes = _lib.SIGNATURES["wu_png_enc_encode"]
    encs = {"none": GPUPngEncoder(dev, threads=threads), "lz77": GPUPngEncoder(dev, threads=threads, matching="lz77")}
    natural = torch.from_numpy(natural_images(16, 512)).to(dev)
    tables = torch.from_numpy(demo_table_batch(8, 4, 6, 256)).to(dev)
    out = {}
    for key, x in (("natural_512x512_b16", natural), (f"demo_tables_{tables.shape[1]}x{tables.shape[2]}_b8", tables)):
        n, h, w, _ = x.shape
        files = {k: e.encode_batch(x) for k, e in encs.items()}          # also uploads the descriptors
        sizes = {k: sum(map(len, f)) / n for k, f in files.items()}
        plan = encs["lz77"]._plan(n, h, w, [(h, w)] * n)                   # the larger workspace serves all three paths
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=dev)
        outb = torch.empty(n * plan.out_stride, dtype=torch.uint8, device=dev)
        result = torch.empty(n, dtype=torch.int32, device=dev)
        st = x.stride()
        new = _lib.load()
        head = (x.data_ptr(), 2, st[0], st[3], st[1], st[2], plan.desc.data_ptr(), ws.data_ptr(), ws.numel(), outb.data_ptr(), outb.numel(),
                result.data_ptr(), n, h, w)

        def chain(fn, *flags):                                             # the same host code around every path: one ctypes call
            def run():
                assert fn(*head, *flags, stream_ptr()) == 0
            return run
        # "none_again" is "none" a second time: what two paths of identical code differ by is the spread of this harness
        paths = {"none": chain(new.wu_png_enc_encode), "none_again": chain(new.wu_png_enc_encode), "lz77": chain(new.wu_png_enc_encode_ex, 1)}
        if old is not None:
            paths = {"parent": chain(old.wu_png_enc_encode), **paths}
            paths["parent"]()
            torch.cuda.synchronize()
            got = [bytes(outb[i * plan.out_stride:i * plan.out_stride + int(result[i])].cpu().numpy()) for i in range(n)]
            assert got == files["none"], "the parent library's files differ from this tree's literal-only files"
            sizes["parent"] = sum(map(len, got)) / n
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t = {k: [] for k in paths}
        for _ in range(3):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        # parent and literal-only alternate among themselves (the matcher's 4 bytes per filtered byte would leave the path after it a
        # cold L2), then LZ77 on its own
        for group in ([k for k in paths if k != "lz77"], ["lz77"]):
            for r in range(21):
                for k in group if r % 2 == 0 else group[::-1]:
                    ev[0].record()
                    paths[k]()
                    ev[1].record()
                    torch.cuda.synchronize()
                    t[k].append(ev[0].elapsed_time(ev[1]) * 1e3)
        out[key] = {"launch_chain_us_events": {k: spread(v) for k, v in t.items()}, "file_bytes_per_image": sizes,
                    "segments": {k: {m: e.stats.get(m, 0) for m in ("stored", "literal", "lz77")} for k, e in encs.items()}}
    for e in encs.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "host", "device", "e2e", "ab"])
    ap.add_argument("--matching", default="none", choices=["none", "lz77"])
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="a run makes whole passes over the images until it has lasted this long")
    a = ap.parse_args()
    import PIL
    from PIL import Image, features
    from wu.infer_driver import class_sweep_to_dir, normalize_minmax, signal_sweep, to_uint8
    from wu.png_enc import GPUPngEncoder

    threads = min(16, a.threads)
    dev = torch.device("cuda:0")
    res = {"cmd": " ".join(sys.argv), "pillow_version": PIL.__version__, "zlib": features.version("zlib"), "cpu": cpu_model(),
           "threads": threads, "images": a.images, "gpu": torch.cuda.get_device_name(0)}
    pool = ThreadPoolExecutor(max_workers=threads)
    enc = GPUPngEncoder(dev, threads=threads, matching=a.matching)
    res["matching"] = a.matching

    def pillow_one(rgb):
        f = io.BytesIO()
        Image.fromarray(rgb).save(f, "PNG")
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
            ref, got = pillow_batch(batches[0]), native_batch(batches[0])             # the same pixels, checked outside the timing
            for r, g in zip(ref, got):
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(r))), np.asarray(Image.open(io.BytesIO(g))))
            key = f"{size}x{size}_b{batch}"
            if a.mode == "device":
                for _ in range(10):
                    enc.launch(batches[0])
                torch.cuda.synchronize()
                res[key] = {"launches": 11}             # the check above + these 10
                continue
            for fn in (pillow_batch, native_batch):
                for b in batches[:2]:
                    fn(b)
            runs = {"pillow": [], "native": []}
            nbytes = {"pillow": 0, "native": 0}
            nfiles = {"pillow": 0, "native": 0}
            for r in range(a.runs):
                order = (("pillow", pillow_batch), ("native", native_batch))
                for name, fn in order if r % 2 == 0 else order[::-1]:
                    w0, c0 = time.perf_counter(), time.process_time()
                    n = 0
                    while n == 0 or time.perf_counter() - w0 < a.min_seconds:      # whole passes; a run of a few ms would measure one hiccup
                        for b in batches:
                            files = fn(b)
                            n += len(files)
                            nbytes[name] += sum(map(len, files))
                            nfiles[name] += len(files)
                    runs[name].append({"images_per_s": n / (time.perf_counter() - w0), "cpu_ms_per_image": 1e3 * (time.process_time() - c0) / n})
            res[key] = {name: {k: spread([v[k] for v in runs[name]]) for k in ("images_per_s", "cpu_ms_per_image")} for name in runs}
            res[key]["file_bytes_per_image"] = {k: nbytes[k] / nfiles[k] for k in nbytes}
            res[key]["file_size_ratio_native_over_pillow"] = (nbytes["native"] / nfiles["native"]) / (nbytes["pillow"] / nfiles["pillow"])
            res[key]["d2h_bytes_per_image"] = {"pillow": size * size * 3, "native": nbytes["native"] / nfiles["native"] + 4}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            t = []
            for _ in range(10):
                ev[0].record()
                enc.launch(batches[0])
                ev[1].record()
                torch.cuda.synchronize()
                t.append(ev[0].elapsed_time(ev[1]) * 1e3)
            res[key]["launch_three_kernels_us_events"] = spread(t)

    if a.mode == "ab":
        res.update(ab(dev, threads))

    if a.mode in ("all", "e2e"):
        import cunet
        from wu.graph_infer import GraphedUNet
        B, S, nc, iters = 16, 512, 5, 1         # one sweep per timing: the serial Pillow writer takes seconds per sweep
        torch.manual_seed(0)
        net = cunet.Conditional_UNet(nc, precision="bf16").to(dev).eval()
        graphed = GraphedUNet(net, B, S)
        batch = (torch.from_numpy(natural_images(B, S)).to(dev).permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
        names = [f"class{i}" for i in range(nc)]
        stems = [f"img{j:04d}" for j in range(B)]
        labels = [j % nc for j in range(B)]
        tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)

        def with_encoder():
            class_sweep_to_dir(net, batch, stems, labels, names, tmp, graphed=graphed, ext=".png", png_encoder=enc)

        def without_encoder():                                         # the same call as it runs today: Pillow, one Image.save per image
            class_sweep_to_dir(net, batch, stems, labels, names, tmp, graphed=graphed, ext=".png")

        def save_one(arg):
            Image.fromarray(arg[0]).save(arg[1])

        def pillow_pool():                                             # ... and with the Pillow saves spread over the 16-thread pool
            rows = torch.eye(nc, device=dev)
            for i in range(nc):
                out = signal_sweep(net, batch, rows[i:i + 1], True, graphed)[0]
                rgb = to_uint8(out).cpu().numpy()
                list(pool.map(save_one, [(rgb[j], os.path.join(tmp, f"{names[labels[j]]}_{stems[j]}_{names[i]}.png")) for j in range(B)]))

        def forward_only():
            rows = torch.eye(nc, device=dev)
            for i in range(nc):
                normalize_minmax(signal_sweep(net, batch, rows[i:i + 1], False, graphed)[0])
            torch.cuda.synchronize()

        order = [("forward_only", forward_only), ("pillow_serial", without_encoder), ("pillow_pool", pillow_pool), ("gpu_encoder", with_encoder)]
        for _, fn in order:
            fn()
        rates = {name: [] for name, _ in order}
        for r in range(min(a.runs, 3)):
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
