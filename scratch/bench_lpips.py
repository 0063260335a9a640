"""Device time of wu.lpips (AlexNet trunk on wu_conv_kxk_fwd / wu_pool3x3_fwd, scaling layer and fused head in csrc/lpips.hip) against the torch
composition of the same numbers on the same GPU: scaling by broadcasting, F.conv2d / F.max_pool2d, then normalise, subtract, square, weight
and mean.

    python scratch/bench_lpips.py [--steps 10] [--warmup 3] [--config sweep class u8] [--precision fp32 bf16]

  sweep   R = 16, B = 16, 3 x 224 x 224, bfloat16 outputs, value range (-1, 1)   (the evaluation sweep)
  class   R = 5,  B = 16, 3 x 512 x 512, float32                                 (the class sweep)
  u8      R = 1,  B = 64, 3 x 224 x 224, uint8 NHWC as a permuted view           (64 decoded pairs)

Per config and model precision one JSON line.  Medians of device events around one call, inputs resident, seeded random weights:
  * ``distance``: LPIPS.distance in passes of at most 64 images, and its torch counterpart with the same passes;
  * ``trunk``: scaling + the five convs and two pools over all (1 + R) B images in those same passes, ours and torch's (torch in the model's dtype:
    float32 convs, or bfloat16 convs under the bf16 model); ``conv1``: the first conv alone over the same images, and its share of the trunk;
  * ``head``: the five layers' head over feature maps held in memory (ours: 10 launches; torch in float64 -- the same numbers -- and in
    float32);
  * ``pairwise`` (R >= 2): LPIPS.pairwise / the torch composition over all i < j;
  * the peak extra device memory of each full call, and how far the torch float64-head distance lies from ours."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIGS = {"sweep": (16, 16, 224, torch.bfloat16, (-1, 1)), "class": (5, 16, 512, torch.float32, (-1, 1)), "u8": (1, 64, 224, torch.uint8, "uint8")}
MAX_IMAGES = 64
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


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
    return round(float(np.median(times)), 3)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


class TorchLPIPS:
    """The composition: the same weights, torch ops only."""

    def __init__(self, model, dev, dtype):
        from wu import lpips
        self.dtype = dtype
        self.convs = []
        for idx, _, _, _, s, p, pool in lpips.ALEX_CONVS:
            m = getattr(model.net.features, str(idx))
            self.convs.append((m.weight.to(dev, dtype), m.bias.to(dev, dtype), s, p, pool))
        self.lin = model.lin_weights(dev)
        self.shift = torch.tensor(SHIFT, device=dev).view(1, 3, 1, 1)
        self.scale = torch.tensor(SCALE, device=dev).view(1, 3, 1, 1)

    def trunk(self, images, s, o, upto=5):
        t = ((images.float() * s + o - self.shift) / self.scale).to(self.dtype)
        outs = []
        for w, b, st, p, pool in self.convs[:upto]:
            if pool:
                t = F.max_pool2d(t, 3, 2)
            t = F.relu(F.conv2d(t, w, b, st, p))
            outs.append(t)
        return outs

    def head(self, fx, fy, k, hdt):
        """fx (B, C, h, w), fy (R, B, C, h, w) -> (R, B)."""
        a, b = fx.to(hdt), fy.to(hdt)
        a = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + 1e-10)
        b = b / (torch.sqrt((b * b).sum(2, keepdim=True)) + 1e-10)
        d = (a.unsqueeze(0) - b) ** 2
        return (d * self.lin[k].to(hdt).view(1, 1, -1, 1, 1)).sum(2).mean((2, 3))

    def distance(self, x, fakes, s, o, hdt=torch.float64):
        r, b = fakes.shape[:2]
        out = torch.zeros(r, b, dtype=hdt, device=x.device)
        fx = self.trunk(x, s, o)
        rows = max(1, MAX_IMAGES // b)
        for r0 in range(0, r, rows):
            nr = min(rows, r - r0)
            fy = self.trunk(fakes[r0:r0 + nr].reshape(nr * b, *fakes.shape[2:]), s, o)
            for k in range(5):
                out[r0:r0 + nr] += self.head(fx[k], fy[k].view(nr, b, *fy[k].shape[1:]), k, hdt)
        return out

    def pairwise(self, fakes, s, o, hdt=torch.float64):
        r, b = fakes.shape[:2]
        step = max(1, MAX_IMAGES // r)
        out = torch.zeros(r, r, b, dtype=hdt, device=fakes.device)
        for b0 in range(0, b, step):
            nb = min(step, b - b0)
            f = self.trunk(fakes[:, b0:b0 + nb].reshape(r * nb, *fakes.shape[2:]), s, o)
            for k in range(5):
                fk = f[k].view(r, nb, *f[k].shape[1:])
                for i in range(r - 1):
                    out[i, i + 1:, b0:b0 + nb] += self.head(fk[i], fk[i + 1:], k, hdt)
        return out + out.transpose(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    a = ap.parse_args()
    from wu import lpips
    from wu.inception import conv_kxk
    from wu.layout import empty_nhwc
    dev = torch.device("cuda:0")
    for name in a.config:
        r, b, size, dt, vr = CONFIGS[name]
        gen = torch.Generator().manual_seed(0)
        x = torch.rand((b, 3, size, size), generator=gen) * 2 - 1
        y = (x.unsqueeze(0) * 0.9 + 0.1 * torch.randn((r, b, 3, size, size), generator=gen)).clamp(-1, 1)
        if dt == torch.uint8:
            x = ((x + 1) * 127.5).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
            y = ((y + 1) * 127.5).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous().to(dev).permute(0, 1, 4, 2, 3)
        else:
            x, y = x.to(dev, dt), y.to(dev, dt)
        s, o = lpips.input_mapping(vr)
        for prec in a.precision:
            model = lpips.LPIPS(prec)
            tdt = torch.float32 if prec == "fp32" else torch.bfloat16
            comp = TorchLPIPS(model, dev, tdt)
            out = {"config": name, "precision": prec, "R": r, "B": b, "size": size, "dtype": str(dt).split(".")[-1], "max_images": MAX_IMAGES,
                   "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
            rows = max(1, MAX_IMAGES // b)
            groups = [(r0, min(rows, r - r0)) for r0 in range(0, r, rows)]          # the passes LPIPS.distance makes: x, then row groups

            def ours_trunk():
                model.features(x, vr)
                for r0, nr in groups:
                    model.features_of_rows(y[r0:r0 + nr], vr)

            def torch_trunk(upto=5):
                comp.trunk(x, s, o, upto)
                for r0, nr in groups:
                    comp.trunk(y[r0:r0 + nr].reshape(nr * b, *y.shape[2:]), s, o, upto)

            def ours_prepare():
                us = [model.prepare(x, vr)]
                for r0, nr in groups:
                    u = empty_nhwc(nr * b, 16, size, size, us[0].dtype, dev)
                    for i in range(nr):
                        model.prepare(y[r0 + i], vr, out=u[i * b:(i + 1) * b])
                    us.append(u)
                return us

            us = ours_prepare()
            p0 = model.net.plan(dev)[0]
            ho, wo = lpips.feature_sizes(size, size)[0]
            y1 = empty_nhwc(max(u.shape[0] for u in us), 64, ho, wo, us[0].dtype, dev)

            def ours_conv1():
                for u in us:
                    conv_kxk(u, p0, y1[:u.shape[0]])

            out["ours_distance_ms"] = timed(lambda: model.distance(x, y, vr, max_images=MAX_IMAGES), a.steps, a.warmup)
            out["ours_distance_peak_extra_bytes"] = peak_extra(lambda: model.distance(x, y, vr, max_images=MAX_IMAGES))
            out["ours_trunk_ms"] = timed(ours_trunk, a.steps, a.warmup)
            out["ours_input_ms"] = timed(ours_prepare, a.steps, a.warmup)
            out["ours_conv1_ms"] = timed(ours_conv1, a.steps, a.warmup)
            out["ours_conv1_share_of_trunk"] = round(out["ours_conv1_ms"] / out["ours_trunk_ms"], 4)
            del us, y1
            out["torch_trunk_ms"] = timed(torch_trunk, a.steps, a.warmup)
            out["torch_conv1_ms"] = timed(lambda: torch_trunk(1), a.steps, a.warmup)
            # heads on held feature maps
            fx = model.features(x, vr)
            fy = model.features_of_rows(y, vr)
            lin = model.lin_weights(dev)
            hout = torch.empty(5, r, b, dtype=torch.float64, device=dev)

            def ours_head():
                for k in range(5):
                    lpips.head(fx[k], fy[k], lin[k], hout[k])

            out["ours_head_ms"] = timed(ours_head, a.steps, a.warmup)
            out["ours_head_peak_extra_bytes"] = peak_extra(ours_head)
            for tag, hdt in (("fp64", torch.float64), ("fp32", torch.float32)):
                fn = lambda: [comp.head(fx[k], fy[k], k, hdt) for k in range(5)]      # noqa: E731
                out[f"torch_head_{tag}_ms"] = timed(fn, a.steps, a.warmup)
                out[f"torch_head_{tag}_peak_extra_bytes"] = peak_extra(fn)
            if r >= 2:
                pout = torch.empty(5, r, r, b, dtype=torch.float64, device=dev)

                def ours_pairs():
                    for k in range(5):
                        lpips.pairs(fy[k], lin[k], pout[k])

                out["ours_pairs_head_ms"] = timed(ours_pairs, a.steps, a.warmup)
            del fx, fy
            torch.cuda.empty_cache()
            ref = model.distance(x, y, vr, max_images=MAX_IMAGES)
            for tag, hdt in (("fp64", torch.float64), ("fp32", torch.float32)):
                fn = lambda: comp.distance(x, y, s, o, hdt)      # noqa: E731
                got = fn()
                out[f"torch_distance_{tag}_ms"] = timed(fn, a.steps, a.warmup)
                out[f"torch_distance_{tag}_peak_extra_bytes"] = peak_extra(fn)
                out[f"torch_distance_{tag}_max_rel_diff"] = float(((got.double() - ref).abs() / ref).max())
            if r >= 2:
                out["ours_pairwise_ms"] = timed(lambda: model.pairwise(y, vr, max_images=MAX_IMAGES), a.steps, a.warmup)
                out["ours_pairwise_peak_extra_bytes"] = peak_extra(lambda: model.pairwise(y, vr, max_images=MAX_IMAGES))
                out["torch_pairwise_fp64_ms"] = timed(lambda: comp.pairwise(y, s, o), max(2, a.steps // 3), 1)
                out["torch_pairwise_fp64_peak_extra_bytes"] = peak_extra(lambda: comp.pairwise(y, s, o))
            out["lpips_mean"] = float(ref.mean())
            print(json.dumps(out), flush=True)
            del model, comp
            torch.cuda.empty_cache()
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
