"""SSIM / MS-SSIM / PSNR / MAE restated in numpy float64: what csrc/ssim.hip and wu/paired.py must compute, operation by operation.

Every numpy expression below rounds each product, sum and quotient on its own (numpy evaluates ``a + g * v`` as two array operations, never
as a fused multiply-add), which is what the kernel does under ``#pragma clang fp contract(off)``; the level-0 ssim map of the kernel must
therefore EQUAL ``maps(...)[0]``.  The means are sums in numpy's (pairwise) order: the kernel's order differs, see ``mean_bound``."""
import numpy as np

U = 2.0 ** -53
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gaussian_window(size=11, sigma=1.5):
    t = np.arange(size, dtype=np.float64)
    g = np.exp(-(t - size // 2) ** 2 / (2.0 * sigma ** 2))
    return g / g.sum()


def range_mapping(value_range):
    """(scale, shift, L): "uint8" -> identity, L = 255; (lo, hi) -> 1 / (hi - lo), -lo scale, L = 1."""
    if value_range == "uint8":
        return 1.0, 0.0, 255.0
    lo, hi = float(value_range[0]), float(value_range[1])
    scale = 1.0 / (hi - lo)
    return scale, -lo * scale, 1.0


def mapped(v, scale, shift):
    """Widen (float32 / uint8 arrays; bfloat16 values arrive as float32, which holds them exactly), then v * scale + shift."""
    v = np.asarray(v).astype(np.float64)
    v = v * scale
    return v + shift


def filter_valid(v, g):
    """Valid filter along axis -2 (H) and then along axis -1 (W), taps in ascending order."""
    k = len(g)
    ho, wo = v.shape[-2] - k + 1, v.shape[-1] - k + 1
    a = g[0] * v[..., 0:ho, :]
    for t in range(1, k):
        a = a + g[t] * v[..., t:t + ho, :]
    b = g[0] * a[..., :, 0:wo]
    for t in range(1, k):
        b = b + g[t] * a[..., :, t:t + wo]
    return b


def maps(x, y, g, c1, c2):
    """(ssim, cs) over the valid positions of mapped float64 images (..., H, W)."""
    mux, muy = filter_valid(x, g), filter_valid(y, g)
    mxx, myy, mxy = mux * mux, muy * muy, mux * muy
    sx = filter_valid(x * x, g) - mxx
    sy = filter_valid(y * y, g) - myy
    sxy = filter_valid(x * y, g) - mxy
    cs = (2.0 * sxy + c2) / ((sx + sy) + c2)
    ssim = ((2.0 * mxy + c1) / ((mxx + myy) + c1)) * cs
    return ssim, cs


def pool(v):
    """2 x 2 mean with size % 2 zero rows / columns in FRONT of an odd dimension: (..., H, W) -> (..., H // 2 + H % 2, W // 2 + W % 2)."""
    ph, pw = v.shape[-2] % 2, v.shape[-1] % 2
    if ph or pw:
        v = np.pad(v, [(0, 0)] * (v.ndim - 2) + [(ph, 0), (pw, 0)])
    p00, p01 = v[..., 0::2, 0::2], v[..., 0::2, 1::2]
    p10, p11 = v[..., 1::2, 0::2], v[..., 1::2, 1::2]
    return ((p00 + p01) + (p10 + p11)) * 0.25


def pooled_sizes(h, w, levels=5):
    out = [(h, w)]
    for _ in range(levels - 1):
        h, w = h // 2 + h % 2, w // 2 + w % 2
        out.append((h, w))
    return out


def pair_stats(x, y, value_range=(-1, 1), win_size=11, sigma=1.5, K=(0.01, 0.03), levels=1, window=None):
    """x (B, C, H, W), y (B, C, H, W) or (R, B, C, H, W) -> dict of float64 arrays with y's leading dimensions:
    ssim_mean, cs_mean (.., C, levels); sse, sae (..); ssim_map, cs_map (.., C, H - k + 1, W - k + 1) of level 0; numel = C H W; L."""
    g = gaussian_window(win_size, sigma) if window is None else np.asarray(window, dtype=np.float64)
    k = len(g)
    scale, shift, L = range_mapping(value_range)
    h, w = x.shape[-2:]
    if levels > 1 and min(h, w) <= (k - 1) * 2 ** (levels - 1):
        raise ValueError(f"MS-SSIM needs min(H, W) > {(k - 1) * 2 ** (levels - 1)}")
    c1, c2 = (K[0] * L) ** 2, (K[1] * L) ** 2
    xm, ym = mapped(x, scale, shift), mapped(y, scale, shift)
    xm = np.broadcast_to(xm, ym.shape)
    d = xm - ym
    out = {"sse": (d * d).sum(axis=(-3, -2, -1)), "sae": np.abs(d).sum(axis=(-3, -2, -1)), "numel": int(np.prod(x.shape[-3:])), "L": L}
    sm, cm = [], []
    for l in range(levels):
        s, c = maps(xm, ym, g, c1, c2)
        if l == 0:
            out["ssim_map"], out["cs_map"] = s, c
        sm.append(s.mean(axis=(-2, -1)))
        cm.append(c.mean(axis=(-2, -1)))
        if l + 1 < levels:
            xm, ym = pool(xm), pool(ym)
    out["ssim_mean"], out["cs_mean"] = np.stack(sm, -1), np.stack(cm, -1)
    return out


def combine_ssim(st, nonnegative=False):
    v = st["ssim_mean"][..., 0]
    if nonnegative:
        v = np.maximum(v, 0.0)
    return v.mean(-1)


def ms_values(ssim_mean, cs_mean):
    """(.., C, levels): the cs means of the first levels, the ssim mean of the last."""
    n = ssim_mean.shape[-1]
    return np.concatenate([cs_mean[..., :n - 1], ssim_mean[..., n - 1:]], -1)


def combine_ms_ssim(st, weights=MS_WEIGHTS):
    v = np.maximum(ms_values(st["ssim_mean"], st["cs_mean"]), 0.0)
    return (v ** np.asarray(weights, dtype=np.float64)).prod(-1).mean(-1)


def mse(st):
    return st["sse"] / st["numel"]


def mae(st):
    return st["sae"] / st["numel"]


def psnr(st):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(st["L"] * st["L"] / mse(st))


def mean_bound(count):
    """|mean of `count` map entries in any order - the same in another order| <= 2 count 2^-53: every entry is at most 1 + 1e-12 in
    magnitude, a sum of n such terms in ANY order carries at most (n - 1) u n (1 + 1e-12) absolute error, two orders differ by twice that,
    and the division by n brings it back to 2 (n - 1) u, plus one rounding of the quotient."""
    return 2.0 * count * U
