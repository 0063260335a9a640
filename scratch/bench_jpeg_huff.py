"""Device Huffman decoding benchmark: GPUJpegDecoder(entropy="device") against entropy="host" in one process, on the workload and
protocol of scratch/bench_jpeg.py (512 generated photo-like JPEGs, 500x375 / 375x500, quality 85, 4:2:0, in memory; batches of 64;
16 host threads; warm-up, then 5 runs of 24 batches per path, the two paths alternating; median and spread).

    python scratch/bench_jpeg_huff.py                                  # link bytes + host comparison + device events + end-to-end line
    python scratch/bench_jpeg_huff.py --mode rounds --files 16         # rounds per chunk from the Python restatement: CPU only
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o huff -- python scratch/bench_jpeg_huff.py --mode device --subseq 1024
                                                                       # kernel times of ONE batch at one subsequence size, a run of its own

Results go to profiles/jpeg_huff_bench.md by hand, with the command line.
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "weather-unet_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_jpeg import cpu_model, make_files, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "host", "device", "e2e", "rounds"])
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--subseq", type=int, default=None, help="subsequence bits of the device path (default: the library's)")
    a = ap.parse_args()
    from wu import jpeg
    from wu.jpeg import GPUJpegDecoder

    S = a.subseq or jpeg.DEFAULT_SUBSEQ_BITS
    threads = min(16, a.threads)
    files = make_files(a.files)
    res = {"cmd": " ".join(sys.argv), "cpu": cpu_model(), "threads": threads, "files": a.files, "batch": a.batch, "subseq_bits": S,
           "mean_file_bytes": sum(map(len, files)) / len(files)}
    batches = [files[i:i + a.batch] for i in range(0, len(files), a.batch)]

    if a.mode == "rounds":                                             # CPU only: the restatement counts what the kernel does not export
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _jpeg_huff_ref as H
        hist = collections.Counter()
        for f in files:
            info = jpeg.parse(f)
            w = H.Walker(H.scan_stage(f, info, S), info, S)
            w.walk()
            hist.update(w.rounds)
        res["rounds_per_chunk_histogram"] = dict(sorted(hist.items()))
        print(json.dumps(res, indent=1))
        return

    res["gpu"] = torch.cuda.get_device_name(0)
    dev = torch.device("cuda:0")
    host = GPUJpegDecoder(dev, threads=threads)
    devd = GPUJpegDecoder(dev, threads=threads, entropy="device", subseq_bits=S)

    def run(dec):
        def fn(items):
            t, _ = dec.decode_batch(items)
            torch.cuda.synchronize()
            return t
        return fn
    host_batch, dev_batch = run(host), run(devd)
    assert torch.equal(host_batch(batches[0]), dev_batch(batches[0]))   # the same tensor, checked once outside the timing
    assert host.stats["fallback"] == 0 and devd.stats["fallback"] == 0

    hb_h, hb_d = host.prepare(batches[0]), devd.prepare(batches[0])
    infos = [jpeg.parse(x) for x in batches[0]]
    staged = [jpeg.scan_stage(x, S) for x in batches[0]]
    res["link_bytes_per_batch"] = {"host_entropy_upload": hb_h.used, "device_entropy_upload": hb_d.used, "device_entropy_status_back": 4 * len(infos),
                                   "coefficients": sum(i.total_blocks for i in infos) * 128,
                                   "scan_bytes_staged": sum(len(s["scan"]) for s in staged), "scan_bytes_bound": sum(s["bound"] for s in staged),
                                   "file_bytes": sum(map(len, batches[0]))}

    if a.mode in ("all", "host"):
        for fn in (host_batch, dev_batch):
            for b in batches[:3]:
                fn(b)
        runs = {"host_entropy": [], "device_entropy": []}
        pair = (("host_entropy", host_batch), ("device_entropy", dev_batch))
        for r in range(a.runs):
            for name, fn in pair if r % 2 == 0 else pair[::-1]:
                w0, c0 = time.perf_counter(), time.process_time()
                n = 0
                for _ in range(a.passes):
                    for b in batches:
                        fn(b)
                        n += len(b)
                runs[name].append({"images_per_s": n / (time.perf_counter() - w0), "cpu_ms_per_image": 1e3 * (time.process_time() - c0) / n})
        for name in runs:
            res[name] = {k: spread([x[k] for x in runs[name]]) for k in ("images_per_s", "cpu_ms_per_image")}
        lib = jpeg._lib.load()
        t0 = time.perf_counter()
        for b in files[:128]:
            jpeg.scan_stage(b, S)
        res["scan_stage_single_thread_ms_per_image_incl_python"] = 1e3 * (time.perf_counter() - t0) / 128
        for name, dec in (("host_entropy", host), ("device_entropy", devd)):
            t0 = time.perf_counter()
            for b in batches[:4]:
                dec.prepare(b).release()
            res[name]["prepare_wall_ms_per_batch"] = 1e3 * (time.perf_counter() - t0) / 4
        del lib

    if a.mode in ("all", "device"):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        out = {}
        for name, dec, hb in (("host_entropy", host, hb_h), ("device_entropy", devd, hb_d)):
            for _ in range(3):
                dec.finish(hb)
            torch.cuda.synchronize()
            t_h2d, t_huff, t_rec = [], [], []
            for _ in range(14):
                ev[0].record()
                db = dec.upload(hb)
                ev[1].record()
                if hb.entropy == "device":
                    dec.huff_decode(db)
                ev[2].record()
                dec.reconstruct(db)
                ev[3].record()
                torch.cuda.synchronize()
                t_h2d.append(ev[0].elapsed_time(ev[1]))
                t_huff.append(ev[1].elapsed_time(ev[2]))
                t_rec.append(ev[2].elapsed_time(ev[3]))
            out[name] = {"h2d_ms": spread(t_h2d), "huff_decode_three_launches_ms": spread(t_huff), "reconstruct_two_launches_ms": spread(t_rec)}
        res["device_events"] = out

    if a.mode in ("all", "e2e"):
        from wu.data import JpegBatchLoader
        from wu.input_pipeline import GPUInputPipeline
        from wu.train_step import WeatherTransferStep
        B, size, iters = 32, 224, 48
        gan = WeatherTransferStep(5, mode="cls", precision="bf16", device=dev, seed=0)
        pipe = GPUInputPipeline(size, augmentation=True, seed=0)
        g = torch.Generator().manual_seed(0)
        x = (torch.rand((B, 3, size, size), generator=g) * 2 - 1).to(dev)
        xr = (torch.rand((B, 3, size, size), generator=g) * 2 - 1).to(dev)
        many = (files * (1 + (2 * B * iters) // len(files)))[:2 * B * iters]

        def resident():
            for _ in range(iters):
                gan.step(x, xr)
            torch.cuda.synchronize()

        def loaded(dec):
            def fn():
                ld = JpegBatchLoader(many, batch_size=2 * B, pipeline=pipe, decoder=dec, prefetch=2)
                for images, _, _ in ld:
                    gan.step(images[:B], images[B:])
                torch.cuda.synchronize()
            return fn
        order = [("resident", resident), ("loader_host_entropy", loaded(host)), ("loader_device_entropy", loaded(devd))]
        for _, fn in order:
            fn()
        rates = {name: [] for name, _ in order}
        for r in range(a.runs):
            for name, fn in order if r % 2 == 0 else order[::-1]:
                t0 = time.perf_counter()
                fn()
                rates[name].append(iters / (time.perf_counter() - t0))
        res["e2e_gan_cls_b32_224_standin_iters_per_s"] = {k: spread(v) for k, v in rates.items()}
        med = {k: statistics.median(v) for k, v in rates.items()}
        res["e2e_ratio_over_resident"] = {k: med[k] / med["resident"] for k in med if k != "resident"}

    hb_h.release()
    hb_d.release()
    host.close()
    devd.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
