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
process keeps a config's allocator state out of the next one's peak.

    python scratch/bench_swd.py --unequal kernel320k [--steps 7] [--warmup 3]

  kernel320k / kernel1m   wu_swd_distance_unequal alone on sorted (512, 64 000) against (512, 320 000) / (512, 1 048 576) float64 columns,
                          against the closed form out of torch ops (int64 arange, two gathers, abs, multiply, sum(1))
  split5x   500 against 2 500 images of 3 x 224 x 224: unequal="exact", the seeded 500-subset rule, the torch composition
  refs5     SlicedWasserstein.compute() of five rows of 500 outputs: five reference banks of 2 500 images, one shared bank, today's inputs
  spread    the subset rule over seeds 0-4 beside the exact value on one pair of sets

The candidates of one --unequal measurement alternate inside every round (`timed_alternating`); a candidate slower than its baseline is
marked LOSS."""
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


# ----------------------------------------------------------------------------------------------
# --unequal: sets of unequal size (wu_swd_distance_unequal, unequal="exact", DescriptorBank, SlicedWasserstein(reference=))
# ----------------------------------------------------------------------------------------------
UNEQUAL = {"kernel320k": (64000, 320000), "kernel1m": (64000, 1 << 20), "split5x": (500, 2500), "refs5": (500, 2500), "spread": (500, 2500)}


def timed_alternating(fns, steps, warmup):
    """{name: (median ms, [all ms])}: the candidates take turns inside every round, so that drift of the machine hits all alike."""
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


def torch_w1_unequal(x, y):
    """The closed form out of torch ops on sorted (ndirs, ml) and (ndirs, ms <= ml) float64 columns: int64 arange, two gathers, abs,
    multiply, sum(1)."""
    ml, ms = x.shape[1], y.shape[1]
    lo = op(torch.arange(ml, device=x.device, dtype=torch.int64) * ms)
    hi = op(lo + ms)
    j0 = op(lo // ml)
    j1 = op(op(hi - 1) // ml)
    mid = op(torch.minimum(hi, op(op(j0 + 1) * ml)))
    w0, w1 = op(op(mid - lo).double()), op(op(hi - mid).double())
    t0 = op(w0 * op(op(x - op(y[:, j0])).abs()))
    t1 = op(w1 * op(op(x - op(y[:, j1])).abs()))
    return op(op(op(t0 + t1).sum(1)) / float(ml * ms))


def _report(out, name, times, baseline):
    for k, (ms, all_ms) in times.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_all"] = ms, all_ms
    for k in times:
        if k != baseline:
            out[f"{k}_vs_{baseline}"] = ("LOSS " if times[k][0] > times[baseline][0] else "") + f"{times[baseline][0] / times[k][0]:.2f}x"
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def bench_unequal_kernel(name, a):
    from wu import _lib
    from wu.layout import stream_ptr
    ms_, ml_ = UNEQUAL[name]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    y = torch.sort(torch.randn((NDIRS, ms_), dtype=torch.float64, device=dev, generator=gen), dim=1)[0]
    x = torch.sort(torch.randn((NDIRS, ml_), dtype=torch.float64, device=dev, generator=gen) * 0.8 + 0.1, dim=1)[0]
    w = torch.empty(NDIRS, dtype=torch.float64, device=dev)

    def fused():
        _lib.call("wu_swd_distance_unequal", y.data_ptr(), ms_, x.data_ptr(), ml_, NDIRS, w.data_ptr(), stream_ptr())
        return w

    def comp():
        return torch_w1_unequal(x, y)

    OPS[0] = 0
    ref = comp()
    ops = OPS[0]
    rel = float(((fused() - ref).abs() / ref).max())
    times = timed_alternating({"fused": fused, "torch": comp}, a.steps, a.warmup)
    nbytes = 8 * NDIRS * (ml_ + ms_)
    out = {"config": name, "ms": ms_, "ml": ml_, "ndirs": NDIRS, "steps": a.steps, "warmup": a.warmup, "torch_op_calls": ops,
           "max_rel_diff": rel, "bytes_read_once": nbytes, "fused_read_GBps": round(nbytes / times["fused"][0] / 1e6, 1),
           "fused_peak_extra_bytes": peak_extra(fused), "torch_peak_extra_bytes": peak_extra(comp)}
    _report(out, name, times, "torch")


def _images(n, size, noise, seed, dev, chunk=500):
    gen = torch.Generator(device=dev).manual_seed(seed)
    parts = []
    for i in range(0, n, chunk):
        k = min(chunk, n - i)
        coarse = torch.rand((k, size // 8, size // 8, 3), generator=gen, device=dev)
        x = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2) * (1 - noise) + noise * torch.rand((k, size, size, 3), generator=gen, device=dev)
        parts.append((x * 255).round().to(torch.uint8))
    return torch.cat(parts).permute(0, 3, 1, 2)                                       # NHWC storage, read through its strides


def bench_unequal_split(name, a):
    """500 against 2 500 images: exact, against the seeded 500-subset of the larger set (what the command line did), against the torch
    composition with the closed form as its last stage."""
    from wu import paired, swd
    na, nb = UNEQUAL[name]
    size, dev = 224, torch.device("cuda:0")
    xa, xb = _images(na, size, 0.3, 0, dev), _images(nb, size, 0.5, 1, dev)
    levels = swd.default_levels(size, size)
    shapes = swd.check_levels(size, size, levels)
    pos, dirs = swd.draw(0, levels, shapes, nb, P, NDIRS)
    pos_d, dirs64 = torch.from_numpy(pos).to(dev), torch.from_numpy(dirs).to(dev).double()
    scale, shift, _ = paired.range_mapping("uint8")
    keep = torch.from_numpy(np.sort(np.random.RandomState(0).permutation(nb)[:na])).to(dev)

    def exact():
        da, db = swd.descriptors(xa, pos[:, :na], "uint8", levels), swd.descriptors(xb, pos, "uint8", levels)
        return swd.distances(da, db, dirs, unequal="exact")

    def subset():
        da, db = swd.descriptors(xa, pos[:, :na], "uint8", levels), swd.descriptors(xb[keep], pos[:, :na], "uint8", levels)
        return swd.distances(da, db, dirs)

    def comp():
        da = torch_descriptors(xa, pos_d[:, :na], levels, scale, shift)
        db = torch_descriptors(xb, pos_d, levels, scale, shift)
        out = []
        for p, q in zip(da, db):
            def cols(dsc):
                v = dsc.double().view(-1, 3, 49)
                mu = v.mean((0, 2), keepdim=True)
                sd = ((v - mu) ** 2).mean((0, 2), keepdim=True).sqrt()
                return torch.sort(dirs64 @ ((v - mu) / sd).float().view(-1, 147).double().t(), dim=1)[0]
            out.append(torch_w1_unequal(cols(q), cols(p)).mean())
        return torch.stack(out)

    fns = {"exact": exact, "subset": subset}
    if not a.no_torch:
        fns["torch"] = comp
    ref = exact()
    out = {"config": name, "images": [na, nb], "size": size, "levels": levels, "P": P, "ndirs": NDIRS, "m": [na * P, nb * P],
           "steps": a.steps, "warmup": a.warmup, "exact_x1e3": [round(float(v) * 1e3, 4) for v in ref.tolist()],
           "subset_x1e3": [round(float(v) * 1e3, 4) for v in subset().tolist()]}
    if not a.no_torch:
        out["max_rel_diff_exact_torch"] = float(((comp() - ref).abs() / ref).max())
    times = timed_alternating(fns, a.steps, a.warmup)
    out.update({f"{k}_peak_extra_bytes": peak_extra(fn) for k, fn in fns.items()})
    for k in ("subset", "torch"):
        if k in times:
            out[f"exact_vs_{k}"] = ("LOSS " if times["exact"][0] > times[k][0] else "") + f"{times[k][0] / times['exact'][0]:.2f}x"
    for k, (ms, all_ms) in times.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_all"] = ms, all_ms
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def bench_unequal_refs(name, a):
    """compute() of SlicedWasserstein over five rows of 500 outputs: each row against its own reference bank of 2 500 images
    (reference=[..]), against one bank shared by the five rows (sorted once per direction group), and today's five rows against the 500
    inputs."""
    from wu import swd
    from wu.evaluate import SlicedWasserstein
    na, nb = UNEQUAL[name]
    size, dev, rows = 224, torch.device("cuda:0"), 5
    banks = []
    for r in range(rows):
        bank = swd.DescriptorBank(P=P, repeats=1, dirs_per_repeat=NDIRS, value_range="uint8")
        for i in range(0, nb, 500):
            bank.add(_images(500, size, 0.35 + 0.05 * r, 100 + 10 * r + i // 500, dev))
        bank.descriptors()
        banks.append(bank)
    xa = _images(na, size, 0.3, 0, dev)
    fakes = torch.stack([_images(na, size, 0.35 + 0.05 * r, 50 + r, dev) for r in range(rows)])
    accs = {"per_class_refs": SlicedWasserstein(P=P, repeats=1, dirs_per_repeat=NDIRS, value_range="uint8", reference=banks),
            "one_shared_ref": SlicedWasserstein(P=P, repeats=1, dirs_per_repeat=NDIRS, value_range="uint8", reference=banks[0]),
            "inputs_today": SlicedWasserstein(P=P, repeats=1, dirs_per_repeat=NDIRS, value_range="uint8")}
    upd = {}
    for k, acc in accs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(0, na, 100):
            acc.update(xa[i:i + 100], fakes[:, i:i + 100])
        e1.record()
        torch.cuda.synchronize()
        upd[k] = round(e0.elapsed_time(e1), 3)
    times = timed_alternating({k: acc.compute for k, acc in accs.items()}, a.steps, a.warmup)
    out = {"config": name, "rows": rows, "outputs_per_row": na, "reference_images": nb, "size": size, "P": P, "ndirs": NDIRS,
           "steps": a.steps, "warmup": a.warmup, "update_ms_once_unwarmed": upd,
           "mean_x1e3": {k: [round(r.mean, 4) for r in acc.compute()] for k, acc in accs.items()}}
    out.update({f"{k}_peak_extra_bytes": peak_extra(acc.compute) for k, acc in accs.items()})
    _report(out, name, times, "inputs_today")


def bench_unequal_spread(name, a):
    """The argument for the feature: on one pair of sets, the subset rule over seeds 0-4 (the seed draws the subset, the positions and the
    directions, as the command line does) beside the exact value over the same seeds (positions and directions only)."""
    from wu import swd
    na, nb = UNEQUAL[name]
    size, dev = 224, torch.device("cuda:0")
    xa, xb = _images(na, size, 0.3, 0, dev), _images(nb, size, 0.5, 1, dev)
    out = {"config": name, "images": [na, nb], "size": size, "P": P, "ndirs": NDIRS, "subset": {}, "exact": {}, "subset_fixed_draws": {}}
    for seed in range(5):
        keep = torch.from_numpy(np.sort(np.random.RandomState(seed).permutation(nb)[:na])).to(dev)
        kw = dict(P=P, repeats=1, dirs_per_repeat=NDIRS, value_range="uint8")
        out["subset"][seed] = [round(v, 4) for v in swd.swd(xa, xb[keep], seed=seed, **kw).levels]
        out["subset_fixed_draws"][seed] = [round(v, 4) for v in swd.swd(xa, xb[keep], seed=0, **kw).levels]
        out["exact"][seed] = [round(v, 4) for v in swd.swd(xa, xb, seed=seed, unequal="exact", **kw).levels]
    for k in ("subset", "subset_fixed_draws", "exact"):
        v = np.array(list(out[k].values()))
        out[f"{k}_min_max_per_level"] = [[float(v[:, l].min()), float(v[:, l].max())] for l in range(v.shape[1])]
        out[f"{k}_mean_min_max"] = [round(float(v.mean(1).min()), 4), round(float(v.mean(1).max()), 4)]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", choices=list(CONFIGS))
    ap.add_argument("--unequal", choices=list(UNEQUAL), help="a measurement on sets of unequal size instead of --config: the distance kernel "
                    "alone (kernel320k, kernel1m), 500 against 2 500 images (split5x), five reference banks (refs5), the subset rule's spread")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (the full configs)")
    a = ap.parse_args()
    if (a.config is None) == (a.unequal is None):
        ap.error("give --config or --unequal")
    if a.unequal:
        {"kernel320k": bench_unequal_kernel, "kernel1m": bench_unequal_kernel, "split5x": bench_unequal_split, "refs5": bench_unequal_refs,
         "spread": bench_unequal_spread}[a.unequal](a.unequal, a)
        return
    (bench_sort if a.config.startswith("sort") else bench_full)(a.config, a)


if __name__ == "__main__":
    main()
