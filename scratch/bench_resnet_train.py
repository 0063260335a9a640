"""ResNet-101 training step (classifier mode: forward, cross-entropy, backward, Adam) at 224 x 224: images/s and ms per step.

    python scratch/bench_resnet_train.py [--batch 16 32] [--steps 20] [--warmup 5] [--impl hip torch-bf16 torch-fp32]

  hip         wu.resnet_train.resnet101(precision="bf16") + wu.estimator_train.EstimatorTrainer: the HIP kernels (train-mode BN,
              weight gradients, per-step weight repacking included in the step)
  torch-bf16  the same network from stock modules (nn.Conv2d(bias=False) / nn.BatchNorm2d / nn.Linear) on the ROCm device, channels-last,
              under torch.autocast(bfloat16): torch's eager path on the same box
  torch-fp32  the same, fp32 throughout

One JSON line per (impl, batch).  For the per-kernel table run it under ``rocprofv3 --kernel-trace --stats`` with one impl."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "weather-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402


class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4)
        self.downsample = None
        if stride != 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return F.relu(out + (self.downsample(x) if self.downsample is not None else x))


class StockResNet101(nn.Module):
    def __init__(self, num_classes=5):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        inplanes, layers = 64, []
        for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 23, 2), (512, 3, 2)):
            mods = []
            for b in range(blocks):
                mods.append(Bottleneck(inplanes, planes, stride if b == 0 else 1))
                inplanes = planes * 4
            layers.append(nn.Sequential(*mods))
        self.layer1, self.layer2, self.layer3, self.layer4 = layers
        self.fc = nn.Linear(2048, num_classes)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


def make_step(impl, dev):
    if impl == "hip":
        from wu.estimator_train import EstimatorTrainer
        from wu.resnet_train import resnet101
        tr = EstimatorTrainer(resnet101(num_classes=5, precision="bf16").to(dev), mode="cls")
        return lambda x, t: tr.step(x, t)[0]
    model = StockResNet101(5).to(dev).to(memory_format=torch.channels_last).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)
    bf16 = impl == "torch-bf16"

    def step(x, t):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            out = model(x.contiguous(memory_format=torch.channels_last))
        loss = F.cross_entropy(out.float(), t)
        loss.backward()
        opt.step()
        return loss.detach()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--impl", nargs="+", default=["hip", "torch-bf16", "torch-fp32"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for impl in a.impl:
        for b in a.batch:
            torch.manual_seed(0)
            step = make_step(impl, dev)
            x = torch.rand((b, 3, a.size, a.size), device=dev) * 2 - 1
            t = torch.randint(0, 5, (b,), device=dev)
            t0 = time.time()
            for _ in range(a.warmup):
                loss = step(x, t)
            torch.cuda.synchronize()
            warm_s = time.time() - t0
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(a.steps):
                loss = step(x, t)
            ev1.record()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / a.steps
            print(json.dumps({"impl": impl, "batch": b, "size": a.size, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3),
                              "images_per_s": round(b * 1000.0 / ms, 1), "loss": round(loss.item(), 4), "warmup_s": round(warm_s, 1),
                              "device": torch.cuda.get_device_name(0)}), flush=True)
            del step, x, t
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
