"""Device time, peak memory and launches of the sliced Wasserstein distance (wu.swd -> csrc/swd.hip) against the composition of the same
numbers out of torch ops on the same GPU: float64 reflect-padded conv2d pyramid, an advanced-index gather of the 3 x 7 x 7 patches, float64
matmul, torch.sort(dim=1), mean absolute difference.

    python scratch/bench_swd.py --config split [--steps 5] [--warmup 2]

  split   500 + 500 images of 3 x 224 x 224 uint8 (NHWC views), 4 levels, 128 patches, 512 directions   (the test split)
  pggan   8192 + 8192 images of 3 x 256 x 256 uint8, 5 levels, 128 patches, 512 directions             (PGGAN's protocol)
  sort64k / sort1m   the sort stage alone: wu_swd_sort_columns on a (512, m) float64 tensor, m = 64 000 / 1 048 576, against torch.sort

One JSON line per config: the median over the timed calls (device events around one whole call, inputs resident), all the times, the peak
device memory above the resident inputs (torch.cuda.max_memory_allocated), the library's launches (counted by `launches`, which mirrors the
launcher's loops) and the composition's torch op calls (each at least one launch), and how far the two results lie apart.  One config per
process keeps a config's allocator state out of the next one's peak."""
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
import torch.nn.functional as F  # noqa: E402

CONFIGS = {"split": (500, 224), "pggan": (8192, 256), "sort64k": 64000, "sort1m": 1 << 20}
P, NDIRS = 128, 512
OPS = [0]


def op(v):
    OPS[0] += 1
    return v


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
    del out
    return torch.cuda.max_memory_allocated() - base


def launches(n, levels, m, ndirs, block):
    """Kernel launches of one swd() call inside the library (the handful of torch ops around them -- mean, stack -- not counted)."""
    from wu import swd
    passes = int(np.ceil(np.log2(max(1, -(-m // block)))))
    chunk = max(1, min(ndirs, (256 << 20) // (8 * m)))
    group = max(1, min(ndirs, swd.PAIR_BYTES // (16 * m)))
    per_sort = sum(-(-min(group, ndirs - g) // min(chunk, group)) for g in range(0, ndirs, group)) * (2 + passes)
    per_level = 2 * 5 + 2 * per_sort + -(-ndirs // group)
    return 2 * (2 * levels - 1) + levels * per_level


def _blur(g, taps):
    c = g.shape[1]
    col = taps.view(1, 1, -1, 1).repeat(c, 1, 1, 1)
    row = taps.view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    v = op(F.conv2d(op(F.pad(g, (0, 0, 2, 2), mode="reflect")), col, groups=c))
    return op(F.conv2d(op(F.pad(v, (2, 2, 0, 0), mode="reflect")), row, groups=c))


def torch_descriptors(x, pos_d, levels, scale, shift):
    f = torch.tensor([1, 4, 6, 4, 1], dtype=torch.float64, device=x.device) / 16
    g = op(op(x.double()) * scale + shift)
    n = x.shape[0]
    out = []
    img = torch.arange(n, device=x.device).view(n, 1, 1, 1, 1)
    ch = torch.arange(3, device=x.device).view(1, 1, 3, 1, 1)
    d = torch.arange(-3, 4, device=x.device)
    for l in range(levels):
        if l == levels - 1:
            lap = g
        else:
            g1 = op(_blur(g, f)[..., ::2, ::2])
            z = op(torch.zeros_like(g))
            z[..., ::2, ::2] = g1
            OPS[0] += 1
            lap = op(g - _blur(z, 2 * f))
        yy = op(pos_d[l, :, :, 0].long().view(n, -1, 1, 1, 1) + d.view(1, 1, 1, 7, 1))
        xx = op(pos_d[l, :, :, 1].long().view(n, -1, 1, 1, 1) + d.view(1, 1, 1, 1, 7))
        out.append(op(op(lap[img, ch, yy, xx]).float().reshape(-1, 147)))
        if l + 1 < levels:
            g = g1
    return out


def torch_level(da, db, dirs64):
    def norm(dsc):
        v = op(dsc.double().view(-1, 3, 49))
        mu = op(v.mean((0, 2), keepdim=True))
        sd = op(op(op(op(v - mu) ** 2).mean((0, 2), keepdim=True)).sqrt())
        return op(op(op(v - mu) / sd).float().view(-1, 147))

    a = op(torch.sort(op(dirs64 @ op(norm(da).double().t())), dim=1)[0])
    b = op(torch.sort(op(dirs64 @ op(norm(db).double().t())), dim=1)[0])
    return op(op(op(a - b).abs()).mean(1)).mean()


def torch_swd(xa, xb, pos_d, dirs64, levels, scale, shift):
    da = torch_descriptors(xa, pos_d, levels, scale, shift)
    db = torch_descriptors(xb, pos_d, levels, scale, shift)
    return torch.stack([torch_level(a, b, dirs64) for a, b in zip(da, db)])


def bench_full(name, a):
    from wu import _lib, paired, swd
    n, size = CONFIGS[name]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    def make(noise):
        coarse = torch.rand((n, size // 8, size // 8, 3), generator=gen, device=dev)
        x = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2) * (1 - noise) + noise * torch.rand((n, size, size, 3), generator=gen, device=dev)
        return (x * 255).round().to(torch.uint8).permute(0, 3, 1, 2)                 # NHWC storage, read through its strides

    xa, xb = make(0.3), make(0.5)
    levels = swd.default_levels(size, size)
    shapes = swd.check_levels(size, size, levels)
    pos, dirs = swd.draw(0, levels, shapes, n, P, NDIRS)
    pos_d = torch.from_numpy(pos).to(dev)
    dirs64 = torch.from_numpy(dirs).to(dev).double()
    scale, shift, _ = paired.range_mapping("uint8")
    m = n * P

    def fused():
        da = swd.descriptors(xa, pos, "uint8", levels)
        db = swd.descriptors(xb, pos, "uint8", levels)
        return swd.distances(da, db, dirs)

    def comp():
        return torch_swd(xa, xb, pos_d, dirs64, levels, scale, shift)

    out = {"config": name, "images_per_set": n, "size": size, "levels": levels, "P": P, "ndirs": NDIRS, "m": m, "steps": a.steps,
           "warmup": a.warmup, "sort_block": _lib.load().wu_swd_sort_block(),
           "fused_launches": launches(n, levels, m, NDIRS, _lib.load().wu_swd_sort_block())}
    ms, all_ms = timed(fused, a.steps, a.warmup)
    out.update(fused_ms_median=round(ms, 3), fused_ms_all=all_ms, fused_peak_extra_bytes=peak_extra(fused))
    ref = fused()
    if not a.no_torch:
        OPS[0] = 0
        got = comp()
        out["torch_op_calls"] = OPS[0]
        out["max_rel_diff"] = float(((got - ref).abs() / ref).max())
        del got
        ms, all_ms = timed(comp, a.steps, a.warmup)
        out.update(torch_ms_median=round(ms, 3), torch_ms_all=all_ms, torch_peak_extra_bytes=peak_extra(comp))
    # where the fused time goes: the stages of the finest level, one at a time
    da, db = swd.descriptors(xa, pos, "uint8", levels), swd.descriptors(xb, pos, "uint8", levels)
    out["stage_descriptors_one_set_ms"] = round(timed(lambda: swd.descriptors(xa, pos, "uint8", levels), a.steps, a.warmup)[0], 3)
    out["stage_normalize_one_level_one_set_ms"] = round(timed(lambda: swd.normalize(da[0]), a.steps, a.warmup)[0], 3)
    na, nb = swd.normalize(da[0])[0], swd.normalize(db[0])[0]
    dirs_d = torch.from_numpy(dirs).to(dev)
    out["stage_project_sort_distance_one_level_ms"] = round(timed(lambda: swd.sliced_wasserstein(na, nb, dirs_d), a.steps, a.warmup)[0], 3)
    out["swd_x1e3"] = [round(float(v) * 1e3, 4) for v in ref.tolist()]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def bench_sort(name, a):
    from wu import _lib, swd
    m = CONFIGS[name]
    dev = torch.device("cuda:0")
    block = _lib.load().wu_swd_sort_block()
    keys = torch.randn((NDIRS, m), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    work = torch.empty_like(keys)

    def fused():
        work.copy_(keys)                          # the sort is in place: the copy is timed on its own below and subtracted
        return swd.sort_columns(work)

    def comp():
        return torch.sort(keys, dim=1)[0]

    copy_ms, _ = timed(lambda: work.copy_(keys), a.steps, a.warmup)
    ms, all_ms = timed(fused, a.steps, a.warmup)
    tms, tall = timed(comp, a.steps, a.warmup)
    same = bool(torch.equal(fused(), comp()))
    passes = int(np.ceil(np.log2(max(1, -(-m // block)))))
    print(json.dumps({"config": name, "m": m, "ncols": NDIRS, "keys": NDIRS * m, "sort_block": block, "steps": a.steps, "warmup": a.warmup,
                      "copy_ms_median": round(copy_ms, 3), "fused_with_copy_ms_median": round(ms, 3), "fused_with_copy_ms_all": all_ms,
                      "fused_sort_ms": round(ms - copy_ms, 3), "fused_launches": 1 + passes + (passes & 1),
                      "fused_peak_extra_bytes": peak_extra(fused), "torch_sort_ms_median": round(tms, 3), "torch_sort_ms_all": tall,
                      "torch_peak_extra_bytes": peak_extra(comp), "equal_to_torch_sort": same,
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", required=True, choices=list(CONFIGS))
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (the full configs)")
    a = ap.parse_args()
    (bench_sort if a.config.startswith("sort") else bench_full)(a.config, a)


if __name__ == "__main__":
    main()
