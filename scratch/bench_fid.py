"""Images/s of the InceptionV3 pool3 pass at 299 x 299 (what FID spends its time on): the HIP path (wu.inception.InceptionV3) against the
same architecture as torch eager ops on the same GPU.

    python scratch/bench_fid.py [--batch 50 100 200] [--steps 10] [--warmup 3] [--impl hip-fp32 hip-bf16 torch-fp32 torch-bf16]

  hip-fp32 / hip-bf16   InceptionV3([3], precision=...): input kernel (uint8 -> 299^2, 2x - 1) + every conv / pool on csrc/inception.hip
  torch-fp32            tests/_inception_ref.py's functional forward (F.conv2d + F.batch_norm + F.relu, avg / max pools, cat) on the GPU,
                        F.interpolate + 2x - 1 in front: torch's eager path (MIOpen convs), channels-last
  torch-bf16            the same under torch.autocast(bfloat16)

Input: a fixed batch of 64 x 64 uint8 images in HBM (the generator-output size of the project), resized to 299 inside the timed pass.
One JSON line per (impl, batch).  For the per-kernel table run it under ``rocprofv3 --kernel-trace --stats`` with one impl."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import _inception_ref as R  # noqa: E402

GFLOP_PER_IMAGE = None


def flops_per_image():
    """2 * MACs of every conv and the fc at 299 x 299 (the pools and the input resize are not counted)."""
    total = 0
    for name, cin, cout, k, s, p in R.CONVS:
        h = R.input_size(name)
        ho = (h + 2 * p[0] - k[0]) // s + 1
        wo = (h + 2 * p[1] - k[1]) // s + 1
        total += 2 * ho * wo * cout * cin * k[0] * k[1]
    return total + 2 * 2048 * 1008


def make_pass(impl, sd, dev):
    if impl.startswith("hip"):
        from wu.inception import InceptionV3
        m = InceptionV3([3], precision=impl.split("-")[1])
        m.load_state_dict(sd)
        return lambda u8: m(u8)[0]
    sdd = {k: v.to(dev) for k, v in sd.items()}
    bf16 = impl == "torch-bf16"

    def run(u8):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            x = u8.permute(0, 3, 1, 2).float().div(255).contiguous(memory_format=torch.channels_last)
            x = R.prepare(x, dtype=torch.float32)
            return R.forward(sdd, x, True, last=3, dtype=torch.float32)[3]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[50, 100, 200])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--impl", nargs="+", default=["hip-fp32", "hip-bf16", "torch-fp32", "torch-bf16"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = R.make_params(True, seed=0)
    fl = flops_per_image()
    for impl in a.impl:
        run = make_pass(impl, sd, dev)
        for b in a.batch:
            g = torch.Generator().manual_seed(b)
            u8 = torch.randint(0, 256, (b, a.size, a.size, 3), generator=g, dtype=torch.uint8).to(dev)
            t0 = time.time()
            for _ in range(a.warmup):
                out = run(u8)
            torch.cuda.synchronize()
            warm_s = time.time() - t0
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(a.steps):
                out = run(u8)
            ev1.record()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / a.steps
            print(json.dumps({"impl": impl, "batch": b, "input": a.size, "steps": a.steps, "warmup": a.warmup, "ms_per_batch": round(ms, 3),
                              "images_per_s": round(b * 1000.0 / ms, 1), "tflops": round(fl * b / ms / 1e9, 1),
                              "gflop_per_image": round(fl / 1e9, 3), "feat_mean": round(out.float().mean().item(), 6),
                              "warmup_s": round(warm_s, 1), "device": torch.cuda.get_device_name(0)}), flush=True)
            del u8, out
        del run
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
