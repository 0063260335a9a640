"""LPIPS (Zhang et al. 2018, net = alex, version 0.1) restated in numpy / torch on the CPU: what wu.lpips and csrc/lpips.hip must compute.
Imports nothing of the HIP library.

Input mapping in float32 with every operation rounded on its own; the trunk by F.conv2d / F.max_pool2d in a chosen dtype; head, pairwise
and diversity on features widened to float64.

The head's arithmetic is carried in numpy's extended precision (64-bit significand) where the platform has it, and the result is rounded
to float64 once: the reference is then the exact value to within half a unit of ITS last place, and ``head_bound`` is a bound on the
kernel's error alone.  On a platform whose long double is a plain double, the reference obeys the same bound as the kernel and
``head_bound`` doubles."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -53
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (state-dict index, cin, cout, k, stride, pad, max pool in front)
CONVS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True), (8, 384, 256, 3, 1, 1, False),
         (10, 256, 256, 3, 1, 1, False))
CHANNELS = tuple(c[2] for c in CONVS)
MIN_SIZE = 31
EPS = 1e-10
WIDE = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64
BOUND_CONST = 12


def input_mapping(value_range):
    """(s, o) of t = v * s + o, as float32."""
    if isinstance(value_range, str):
        assert value_range == "uint8"
        return np.float32(2.0 / 255.0), np.float32(-1.0)
    s, o = {(-1, 1): (1.0, 0.0), (0, 1): (2.0, -1.0)}[tuple(value_range)]
    return np.float32(s), np.float32(o)


def scale_input(v, value_range=(-1, 1)):
    """(..., 3, H, W) array of float32 / uint8 values (bfloat16 values arrive widened to float32) -> float32 u, four roundings per value."""
    s, o = input_mapping(value_range)
    t = np.asarray(v).astype(np.float32)
    t = (t * s).astype(np.float32)
    t = (t + o).astype(np.float32)
    shape = (3, 1, 1)
    t = (t - np.asarray(SHIFT, np.float32).reshape(shape)).astype(np.float32)
    return (t / np.asarray(SCALE, np.float32).reshape(shape)).astype(np.float32)


def network_input(v, value_range=(-1, 1), bf16=False):
    """The (N, H, W, 16) network input as a torch tensor in the storage dtype: scale_input, rounded to bfloat16 if asked, channels 3..15 zero."""
    u = torch.from_numpy(scale_input(v, value_range))
    n, _, h, w = u.shape
    out = torch.zeros(n, h, w, 16, dtype=torch.float32)
    out[..., :3] = u.permute(0, 2, 3, 1)
    return out.to(torch.bfloat16) if bf16 else out


def make_params(seed):
    """(alexnet state-dict with torchvision's keys, lin state-dict with the lpips package's keys): He-normal conv weights, small random
    biases, lin weights uniform in [0, 1).  Values without meaning: they exercise the arithmetic."""
    g = torch.Generator().manual_seed(seed)
    alex, lin = {}, {}
    for k, (idx, cin, cout, ks, _, _, _) in enumerate(CONVS):
        alex[f"features.{idx}.weight"] = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        alex[f"features.{idx}.bias"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
        lin[f"lin{k}.model.1.weight"] = torch.rand(1, cout, 1, 1, generator=g)
    return alex, lin


def feature_sizes(h, w):
    if min(h, w) < MIN_SIZE:
        raise ValueError(f"LPIPS (alex) needs min(H, W) >= {MIN_SIZE}, got {h} x {w}")
    out = []
    for _, _, _, k, s, p, pool in CONVS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((h, w))
    return out


def trunk(alex, u, dtype=torch.float64, bf16=False):
    """The five ReLU outputs [(N, C_k, h_k, w_k)] of u (N, 3, H, W) float32 (scale_input's result).  ``dtype`` is the arithmetic of
    F.conv2d; with bf16=True the input, the weights and every stored activation are rounded to bfloat16 (bias and accumulation stay in
    ``dtype``): a CPU model of the bf16 storage mode."""
    feature_sizes(*u.shape[-2:])

    def rnd(t):
        return t.to(torch.bfloat16).to(dtype) if bf16 else t

    t = rnd(torch.as_tensor(u).to(dtype))
    outs = []
    for idx, _, _, _, s, p, pool in CONVS:
        if pool:
            t = F.max_pool2d(t, 3, 2)
        w = rnd(alex[f"features.{idx}.weight"].to(dtype))
        t = rnd(F.relu(F.conv2d(t, w, alex[f"features.{idx}.bias"].to(dtype), s, p)))
        outs.append(t)
    return outs


def _np(t):
    return t.detach().to(torch.float64).numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def unit(f):
    """(..., C, h, w) -> f / (norm over C + 1e-10) in the wide type."""
    f = _np(f).astype(WIDE)
    n = np.sqrt((f * f).sum(axis=-3, keepdims=True))
    return f / (n + WIDE(EPS))


def head(fa, fb, w):
    """One layer: fa (..., C, h, w) against fb (broadcastable, e.g. (R, B, C, h, w)), w (C,) -> float64 (...)."""
    a, b = unit(fa), unit(fb)
    d = a - b
    wv = _np(w).reshape(-1).astype(WIDE).reshape(-1, 1, 1)
    hw = d.shape[-1] * d.shape[-2]
    return ((wv * (d * d)).sum(axis=(-3, -2, -1)) / WIDE(hw)).astype(np.float64)


def head_bound(fa, fb, w):
    """Bound on |kernel - head(fa, fb, w)| per entry, derived, not measured.  u = 2^-53, S_c = |ah_c| + |bh_c|.

    Norm: C products (1 rounding each) and C - 1 additions of non-negative terms, in any order: relative error <= C u; the square root halves
    it and rounds once, the addition of 1e-10 and the division round once each: ah_c carries a relative error e_n <= (C / 2 + 3) u.
    Difference: |ah_c| e_n + |bh_c| e_n + u |ah_c - bh_c| <= (e_n + u) S_c.  Square: 2 |d| (e_n + u) S_c + u d^2 <= (2 e_n + 3 u) S_c^2.
    Times w_c: one more u.  Sum over the channels, any order: (C - 1) u on sum_c |w_c| S_c^2.  Sum over the h w pixels, any order, in
    workgroup partial sums and their fold: (h w - 1) u.  Division by h w: u.  Together
        (2 (C / 2 + 3) + 3 + 1 + (C - 1) + (h w - 1) + 1) u = (2 C + h w + 9) u
    times M = mean over the pixels of sum_c |w_c| S_c^2.  The constant 12 covers the 9, the reference's own rounding to float64 (u / 2 of
    |ref| <= M) and the second-order terms of (1 + u)^n for n <= 2 C + h w + 9 < 2^20."""
    a, b = np.abs(unit(fa)), np.abs(unit(fb))
    c, h, wd = a.shape[-3:]
    wv = np.abs(_np(w).reshape(-1)).astype(WIDE).reshape(-1, 1, 1)
    m = ((wv * (a + b) ** 2).sum(axis=(-3, -2, -1)) / (h * wd)).astype(np.float64)
    sides = 1 if WIDE is not np.float64 else 2
    return sides * (2 * c + h * wd + BOUND_CONST) * U * m


def total(layers):
    """(((d_1 + d_2) + d_3) + d_4) + d_5 of (..., 5)."""
    layers = np.asarray(layers, np.float64)
    return (((layers[..., 0] + layers[..., 1]) + layers[..., 2]) + layers[..., 3]) + layers[..., 4]


def distance_layers(fx, fy, lin):
    """fx: five (B, C_k, h, w); fy: five (R, B, C_k, h, w) -> (R, B, 5) float64."""
    return np.stack([head(_np(fx[k])[None], fy[k], lin[f"lin{k}.model.1.weight"]) for k in range(5)], -1)


def pairwise_layers(f, lin):
    """f: five (R, B, C_k, h, w) -> (R, R, B, 5) float64; entry (i, j) is head(row i, row j)."""
    return np.stack([head(_np(f[k])[:, None], _np(f[k])[None], lin[f"lin{k}.model.1.weight"]) for k in range(5)], -1)


def diversity(pair_matrix):
    """(R, R, B) -> (B,): the mean over i < j."""
    r = pair_matrix.shape[0]
    iu = np.triu_indices(r, 1)
    return pair_matrix[iu].sum(0) / (r * (r - 1) // 2)


def features(alex, images, value_range=(-1, 1), dtype=torch.float64, bf16=False):
    """Five feature maps of (..., 3, H, W) images, leading dimensions kept."""
    images = np.asarray(images)
    lead = images.shape[:-3]
    u = torch.from_numpy(scale_input(images.reshape((-1,) + images.shape[-3:]), value_range))
    return [f.reshape(lead + tuple(f.shape[1:])) for f in trunk(alex, u, dtype, bf16)]


def lpips(alex, lin, x, fakes, value_range=(-1, 1), dtype=torch.float64, bf16=False):
    """{"layers" (R, B, 5), "distance" (R, B), "pair_layers" (R, R, B, 5), "pairwise" (R, R, B), "diversity" (B,) or None, "min_norm"} of
    x (B, 3, H, W) and fakes (R, B, 3, H, W)."""
    fx, fy = features(alex, x, value_range, dtype, bf16), features(alex, fakes, value_range, dtype, bf16)
    layers = distance_layers(fx, fy, lin)
    pl = pairwise_layers(fy, lin)
    pw = total(pl)
    min_norm = min(float(np.sqrt((_np(f) ** 2).sum(axis=-3)).min()) for f in fx + fy)
    return {"layers": layers, "distance": total(layers), "pair_layers": pl, "pairwise": pw,
            "diversity": diversity(pw) if pw.shape[0] >= 2 else None, "min_norm": min_norm}
