"""Float64 CPU restatement of InceptionV3 (torchvision's Inception3 and pytorch-fid's FID variant) in plain torch.nn.functional ops,
for the tests of wu.inception / wu.fid.  Written from the architecture alone; no torchvision.

    make_params(fid, seed)         seeded synthetic state-dict with torchvision's key names (conv weights He-scaled, BatchNorm gamma ~ 1,
                                   beta / running mean small, running_var ~ 1: activations stay O(1) through all the layers)
    prepare(images, resize, normalize)   (N,3,H,W) float in [0, 1] -> bilinear 299 x 299 (align_corners=False) -> 2x - 1, float64
    forward(sd, x, fid, last=3)    {0: block 0, 1: block 1, 2: block 2, 3: (N, 2048) pool3, "logits": (N, classes)} up to block `last`
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-3


# (name, cin, cout, kernel, stride, padding) of every BasicConv2d, torchvision's Inception3 order
def _a(m, cin, pf):
    return [(f"{m}.branch1x1", cin, 64, (1, 1), 1, (0, 0)), (f"{m}.branch5x5_1", cin, 48, (1, 1), 1, (0, 0)),
            (f"{m}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2)), (f"{m}.branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (f"{m}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (f"{m}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)),
            (f"{m}.branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def _b(m, cin):
    return [(f"{m}.branch3x3", cin, 384, (3, 3), 2, (0, 0)), (f"{m}.branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (f"{m}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (f"{m}.branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _c(m, cin, c7):
    r, c = ((1, 7), (0, 3)), ((7, 1), (3, 0))
    return [(f"{m}.branch1x1", cin, 192, (1, 1), 1, (0, 0)), (f"{m}.branch7x7_1", cin, c7, (1, 1), 1, (0, 0)),
            (f"{m}.branch7x7_2", c7, c7, r[0], 1, r[1]), (f"{m}.branch7x7_3", c7, 192, c[0], 1, c[1]),
            (f"{m}.branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), (f"{m}.branch7x7dbl_2", c7, c7, c[0], 1, c[1]),
            (f"{m}.branch7x7dbl_3", c7, c7, r[0], 1, r[1]), (f"{m}.branch7x7dbl_4", c7, c7, c[0], 1, c[1]),
            (f"{m}.branch7x7dbl_5", c7, 192, r[0], 1, r[1]), (f"{m}.branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def _d(m, cin):
    return [(f"{m}.branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), (f"{m}.branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            (f"{m}.branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)), (f"{m}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            (f"{m}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), (f"{m}.branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _e(m, cin):
    return [(f"{m}.branch1x1", cin, 320, (1, 1), 1, (0, 0)), (f"{m}.branch3x3_1", cin, 384, (1, 1), 1, (0, 0)),
            (f"{m}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), (f"{m}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            (f"{m}.branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), (f"{m}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            (f"{m}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), (f"{m}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            (f"{m}.branch_pool", cin, 192, (1, 1), 1, (0, 0))]


CONVS = ([("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)),
          ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)), ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)),
          ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]
         + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64) + _b("Mixed_6a", 288)
         + _c("Mixed_6b", 768, 128) + _c("Mixed_6c", 768, 160) + _c("Mixed_6d", 768, 160) + _c("Mixed_6e", 768, 192)
         + _d("Mixed_7a", 768) + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
SPEC = {c[0]: c for c in CONVS}
# input resolution of every conv at a 299 x 299 network input
_RES = {"Conv2d_1a_3x3": 299, "Conv2d_2a_3x3": 149, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 73,
        "Mixed_5": 35, "Mixed_6a": 35, "Mixed_6": 17, "Mixed_7a": 17, "Mixed_7": 8}


def input_size(name):
    for k in (name, name.split(".")[0], name[:7]):
        if k in _RES:
            return _RES[k]
    raise KeyError(name)


def num_classes(fid):
    return 1008 if fid else 1000


def make_params(fid=True, seed=0, num_batches_tracked=True):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, k, _, _ in CONVS:
        fan_in = cin * k[0] * k[1]
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, *k, generator=g) * (2.0 / fan_in) ** 0.5
        sd[f"{name}.bn.weight"] = 1.0 + 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 1.0 + 0.2 * torch.rand(cout, generator=g)
        if num_batches_tracked:
            sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    nc = num_classes(fid)
    sd["fc.weight"] = torch.randn(nc, 2048, generator=g) * (1.0 / 2048) ** 0.5
    sd["fc.bias"] = 0.01 * torch.randn(nc, generator=g)
    return sd


def prepare(images, resize=True, normalize=True, dtype=torch.float64):
    x = images.to(dtype)
    if resize:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    return 2 * x - 1 if normalize else x


def forward(sd, x, fid=True, last=3, dtype=torch.float64):
    """x: the network input (after prepare), NCHW; computed in `dtype` on x's device (float64 on the CPU = the reference)."""
    sd = {k: v.to(device=x.device, dtype=dtype) if v.is_floating_point() else v for k, v in sd.items()}

    def bc(name, t):
        _, _, _, _, s, p = SPEC[name]
        y = F.conv2d(t, sd[f"{name}.conv.weight"], None, s, p)
        y = F.batch_norm(y, sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"], sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"],
                         False, 0.0, BN_EPS)
        return F.relu(y)

    def avg(t):
        return F.avg_pool2d(t, 3, 1, 1, count_include_pad=not fid)

    def mixed_a(m, t):
        b1 = bc(f"{m}.branch1x1", t)
        b5 = bc(f"{m}.branch5x5_2", bc(f"{m}.branch5x5_1", t))
        b3 = bc(f"{m}.branch3x3dbl_3", bc(f"{m}.branch3x3dbl_2", bc(f"{m}.branch3x3dbl_1", t)))
        return torch.cat([b1, b5, b3, bc(f"{m}.branch_pool", avg(t))], 1)

    def mixed_b(m, t):
        b3 = bc(f"{m}.branch3x3", t)
        bd = bc(f"{m}.branch3x3dbl_3", bc(f"{m}.branch3x3dbl_2", bc(f"{m}.branch3x3dbl_1", t)))
        return torch.cat([b3, bd, F.max_pool2d(t, 3, 2)], 1)

    def mixed_c(m, t):
        b1 = bc(f"{m}.branch1x1", t)
        b7 = bc(f"{m}.branch7x7_3", bc(f"{m}.branch7x7_2", bc(f"{m}.branch7x7_1", t)))
        bd = t
        for i in range(1, 6):
            bd = bc(f"{m}.branch7x7dbl_{i}", bd)
        return torch.cat([b1, b7, bd, bc(f"{m}.branch_pool", avg(t))], 1)

    def mixed_d(m, t):
        b3 = bc(f"{m}.branch3x3_2", bc(f"{m}.branch3x3_1", t))
        b7 = t
        for i in range(1, 5):
            b7 = bc(f"{m}.branch7x7x3_{i}", b7)
        return torch.cat([b3, b7, F.max_pool2d(t, 3, 2)], 1)

    def mixed_e(m, t, maxpool):
        b1 = bc(f"{m}.branch1x1", t)
        u = bc(f"{m}.branch3x3_1", t)
        b3 = torch.cat([bc(f"{m}.branch3x3_2a", u), bc(f"{m}.branch3x3_2b", u)], 1)
        u = bc(f"{m}.branch3x3dbl_2", bc(f"{m}.branch3x3dbl_1", t))
        bd = torch.cat([bc(f"{m}.branch3x3dbl_3a", u), bc(f"{m}.branch3x3dbl_3b", u)], 1)
        p = F.max_pool2d(t, 3, 1, 1) if maxpool else F.avg_pool2d(t, 3, 1, 1, count_include_pad=not fid)
        return torch.cat([b1, b3, bd, bc(f"{m}.branch_pool", p)], 1)

    out = {}
    x = F.max_pool2d(bc("Conv2d_2b_3x3", bc("Conv2d_2a_3x3", bc("Conv2d_1a_3x3", x))), 3, 2)
    out[0] = x
    if last >= 1:
        x = F.max_pool2d(bc("Conv2d_4a_3x3", bc("Conv2d_3b_1x1", x)), 3, 2)
        out[1] = x
    if last >= 2:
        for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = mixed_a(m, x)
        x = mixed_b("Mixed_6a", x)
        for m in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = mixed_c(m, x)
        out[2] = x
    if last >= 3:
        x = mixed_d("Mixed_7a", x)
        x = mixed_e("Mixed_7b", x, False)
        x = mixed_e("Mixed_7c", x, fid)
        feat = x.mean(dim=(2, 3))
        out[3] = feat
        out["logits"] = F.linear(feat, sd["fc.weight"], sd["fc.bias"])
    return out
