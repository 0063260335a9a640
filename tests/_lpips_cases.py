"""The case list shared by tests/test_lpips_cpu.py and tests/test_gpu_lpips.py.  CPU work on small tensors; imports nothing of the HIP library."""
import numpy as np
import torch

INPUT_SIZES = ((31, 31), (33, 47))
HEAD_CHANNELS = (16, 64, 192, 256, 384)
HEAD_MAPS = ((1, 1), (3, 5), (13, 13))
HEAD_ROWS = (1, 3)
HEAD_B = 2
PAIR_ROWS = (2, 3, 16)
E2E_SIZES = ((31, 31), (31, 47), (67, 35), (64, 64))
E2E_ROWS = (1, 3)
E2E_B = 2
PARAM_SEED = 5

# AlexNet's trunk configurations at the smallest maps that still have a border and an interior, for the exact integer oracle:
# (name, n, h, w, cin, cin_w, cout, k, stride, pad)
TRUNK_CONVS = (("conv1", 2, 31, 35, 16, 3, 64, 11, 4, 2), ("conv2", 2, 7, 9, 64, 64, 192, 5, 1, 2), ("conv3", 2, 3, 4, 192, 192, 384, 3, 1, 1),
               ("conv4", 2, 3, 4, 384, 384, 256, 3, 1, 1), ("conv5", 2, 3, 4, 256, 256, 256, 3, 1, 1),
               ("conv3_1x1", 3, 1, 1, 192, 192, 384, 3, 1, 1), ("conv4_1x1", 3, 1, 1, 384, 384, 256, 3, 1, 1),
               ("conv5_1x1", 3, 1, 1, 256, 256, 256, 3, 1, 1))
TRUNK_POOLS = ((2, 64, 7, 9), (2, 192, 3, 4), (2, 64, 15, 15))          # (n, c, h, w): 3 x 3 stride 2 -> 3 x 4, 1 x 1, 7 x 7


def head_pixel_maps(tile):
    """The (h, w) of the head cases: the fixed maps and pixel counts one below, at and one above the kernel's pixels per workgroup."""
    return HEAD_MAPS + ((1, tile - 1), (1, tile), (tile + 1, 1))


def trunk_operands(case):
    """Integer operands (int64): x in [-4, 4] in ALL cin channels (the packed weight is zero past cin_w), w in [-2, 2], bias in [-8, 8].
    K <= 3456, so every partial sum stays below 3456 * 8 + 8 < 2^24 and fp32 accumulation is exact in any order."""
    name, n, h, w, cin, cin_w, cout, k, s, p = case
    assert k * k * cin * 8 + 8 < 2 ** 24
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randint(-4, 5, (n, cin, h, w), generator=g)
    wt = torch.randint(-2, 3, (cout, cin_w, k, k), generator=g)
    b = torch.randint(-8, 9, (cout,), generator=g)
    return x, wt, b


def trunk_expected(case):
    """relu(conv + bias) in int64, by unfolding: exact."""
    name, n, h, w, cin, cin_w, cout, k, s, p = case
    x, wt, b = trunk_operands(case)
    xp = torch.nn.functional.pad(x[:, :cin_w], (p, p, p, p))
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    out = torch.zeros(n, cout, ho, wo, dtype=torch.int64)
    for i in range(k):
        for j in range(k):
            patch = xp[:, :, i:i + s * (ho - 1) + 1:s, j:j + s * (wo - 1) + 1:s]                 # (n, cin_w, ho, wo)
            out += torch.einsum("nchw,oc->nohw", patch, wt[:, :, i, j])
    return torch.clamp(out + b.view(1, -1, 1, 1), min=0)


def feature_maps(c, h, w, rows, b, seed, zeros=True):
    """ReLU-like float32 feature maps x (B, C, h, w), y (R, B, C, h, w): half the entries zero, y a perturbed x.  With ``zeros`` (and more
    than 3 pixels) pixel 0 of x, pixel 1 of the y rows and pixel 2 of both hold exact zero vectors; then row 0 of y is made x bit for bit where R > 1."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.normal(size=(b, c, h, w)), 0).astype(np.float32)
    y = np.maximum(x[None] + 0.5 * rng.normal(size=(rows, b, c, h, w)), 0).astype(np.float32)
    if zeros and h * w > 3:
        xf, yf = x.reshape(b, c, h * w), y.reshape(rows, b, c, h * w)
        xf[:, :, 0] = 0
        yf[:, :, :, 1] = 0
        xf[:, :, 2] = 0
        yf[:, :, :, 2] = 0
    if rows > 1:
        y[0] = x
    return x, y


def lin_weight(c, seed):
    """(C,) float32 of both signs."""
    w = np.random.default_rng(1000 + seed).normal(size=c).astype(np.float32)
    assert (w > 0).any() and (w < 0).any()
    return w


def images(b, rows, h, w, seed):
    """Uniform-noise images in [-1, 1]: x (B, 3, H, W) and fakes (R, B, 3, H, W), each fake half x and half fresh noise.  float32."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(b, 3, h, w)).astype(np.float32)
    fakes = (0.5 * x[None] + 0.5 * rng.uniform(-1, 1, size=(rows, b, 3, h, w))).astype(np.float32)
    return x, fakes


def e2e_cases():
    return [(h, w, r) for h, w in E2E_SIZES for r in E2E_ROWS]


def e2e_seed(h, w, r):
    return 10000 * h + 10 * w + r
