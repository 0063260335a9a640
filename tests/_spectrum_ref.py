"""The radial power-spectrum metric of wu/spectrum.py, restated with numpy and Python integers only: the oracle of tests/test_spectrum_cpu.py
and tests/test_gpu_spectrum.py.  Every product and sum is an elementwise fp64 numpy operation, rounded on its own; inner products are
accumulated term by term in ascending index order."""
import math

import numpy as np

U = 2.0 ** -53


def range_mapping(value_range):
    if isinstance(value_range, str):
        assert value_range == "uint8"
        return 1.0, 0.0, 255.0
    lo, hi = (float(v) for v in value_range)
    scale = 1.0 / (hi - lo)
    return scale, -lo * scale, 1.0


def twiddles(n):
    """(c, s): cos and sin of 2 pi k / n for k < n, from an argument reduced to [0, pi / 4] in integers."""
    c, s = np.empty(n), np.empty(n)
    for k in range(n):
        q, r = divmod(8 * k, n)
        if q % 2 == 0:
            a = (r / n) * (math.pi / 4)
            ck, sk = math.cos(a), math.sin(a)
        else:
            a = ((n - r) / n) * (math.pi / 4)
            ck, sk = math.sin(a), math.cos(a)
        for _ in range(q // 2):
            ck, sk = -sk, ck
        c[k], s[k] = ck, sk
    return c + 0.0, s + 0.0          # -0.0 -> +0.0


def hann(n):
    return 0.5 - 0.5 * twiddles(n)[0]


def luma(x, value_range=(-1, 1), window="none"):
    """x (N, C, H, W) of any numpy dtype whose values are exact in float64 -> (N, H, W) float64."""
    scale, shift, L = range_mapping(value_range)
    s = (x.astype(np.float64) * scale + shift) / L
    if x.shape[1] == 3:
        y = (0.299 * s[:, 0] + 0.587 * s[:, 1]) + 0.114 * s[:, 2]
    else:
        assert x.shape[1] == 1
        y = s[:, 0]
    if window == "hann":
        y = (y * hann(x.shape[2])[None, :, None]) * hann(x.shape[3])[None, None, :]
    else:
        assert window == "none"
    return y


def half_spectrum(y):
    """(Xr, Xi) of shape (N, H, Wh) from planes (N, H, W): the two stages of the definition, terms added in ascending order."""
    n, h, w = y.shape
    wh = w // 2 + 1
    cw, sw = twiddles(w)
    ch, sh = twiddles(h)
    v = np.arange(wh)
    tr, ti = np.zeros((n, h, wh)), np.zeros((n, h, wh))
    for j in range(w):
        at = (v * j) % w
        tr = tr + y[:, :, j, None] * cw[at]
        ti = ti + y[:, :, j, None] * sw[at]
    ti = -ti
    u = np.arange(h)
    xr, xi = np.zeros((n, h, wh)), np.zeros((n, h, wh))
    for i in range(h):
        at = (u * i) % h
        c, s = ch[at][None, :, None], sh[at][None, :, None]
        xr = xr + (c * tr[:, i, None, :] + s * ti[:, i, None, :])
        xi = xi + (c * ti[:, i, None, :] - s * tr[:, i, None, :])
    return xr, xi


def mirror_weights(w):
    v = np.arange(w // 2 + 1)
    return np.where((v > 0) & (2 * v < w), 2, 1).astype(np.int64)


def radial_bins(h, w):
    """(bin (H, Wh) int32, count (K,) int64, freq (K,) float64): Python integers throughout."""
    wh, m = w // 2 + 1, min(h, w)
    idx = np.empty((h, wh), dtype=np.int32)
    for u in range(h):
        fu = u if u <= h // 2 else u - h
        for v in range(wh):
            q = fu * fu * w * w + v * v * h * h
            idx[u, v] = math.isqrt(q * m * m) // (h * w)
    K = int(idx.max()) + 1
    count = np.zeros(K, dtype=np.int64)
    np.add.at(count, idx, np.broadcast_to(mirror_weights(w), (h, wh)))
    return idx, count, np.arange(K) / m


def profiles_planes(y):
    """prof (N, K) and P (N, H, Wh) of planes (N, H, W)."""
    n, h, w = y.shape
    xr, xi = half_spectrum(y)
    p = xr * xr + xi * xi
    idx, count, _ = radial_bins(h, w)
    wp = p * mirror_weights(w).astype(np.float64)
    K = count.shape[0]
    sums = np.zeros((n, K))
    flat_idx, flat = idx.reshape(-1), wp.reshape(n, -1)
    for k in range(K):
        for e in np.nonzero(flat_idx == k)[0]:
            sums[:, k] = sums[:, k] + flat[:, e]
    hw2 = float(h * w) * float(h * w)
    return sums / count.astype(np.float64) / hw2, p


def profiles(x, value_range=(-1, 1), window="none"):
    return profiles_planes(luma(x, value_range, window))[0]


def mean_spectrum(p):
    """mean_n P[n] / (H W)^2 for P (N, H, Wh) of an H x W image set, summed over n ascending."""
    n, h, wh = p.shape
    s = np.zeros((h, wh))
    for i in range(n):
        s = s + p[i]
    return s, n


# ---- everything after the profiles: (N, K)-sized arithmetic -------------------------------------------------------------------------------
def bank_stats(prof, m):
    """(sum dB (K,), sum dB^2 (K,), images kept, flat) of profiles (N, K); an image with a bin of zero power in 1 .. m // 2 is flat."""
    lo, hi = 1, m // 2
    flat = np.any(prof[:, lo:hi + 1] == 0.0, axis=1) if hi >= lo else np.zeros(prof.shape[0], dtype=bool)
    keep = prof[~flat]
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(keep)
    return db.sum(0), (db * db).sum(0), keep.shape[0], int(flat.sum())


def compare(stats_a, stats_b, m):
    """The entries of SpectrumResult from two bank_stats tuples, over bins 1 .. m // 2."""
    lo, hi = 1, m // 2
    out = {}
    for tag, (s1, s2, cnt, _) in (("a", stats_a), ("b", stats_b)):
        mean = s1[lo:hi + 1] / cnt
        var = s2[lo:hi + 1] / cnt - mean * mean
        out["mean_db_" + tag] = mean
        out["std_db_" + tag] = np.sqrt(np.maximum(var, 0.0))
    d = out["mean_db_b"] - out["mean_db_a"]
    nb = d.shape[0]
    out["freq"] = np.arange(lo, hi + 1) / m
    out["lsd"] = float(np.sqrt(np.mean(d * d))) if nb else float("nan")
    t1, t2 = nb // 3, (2 * nb) // 3
    out["bands"] = tuple(float(np.mean(seg)) if seg.shape[0] else float("nan") for seg in (d[:t1], d[t1:t2], d[t2:]))
    if nb:
        at = int(np.argmax(np.abs(d)))
        out["peak"] = (float(np.abs(d[at])), float(out["freq"][at]))
    else:
        out["peak"] = (float("nan"), float("nan"))
    return out
