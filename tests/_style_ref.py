"""CPU oracles for csrc/adain_style.hip (wu_adain_style_{fwd,bwd} and their _multi forms).  numpy / torch only, nothing from wu.

    forward   y4 = (y W^T + b).view(N, C, 4);  y_mean = mean_k y4;  y_std = sqrt(var_k(y4, unbiased) + eps)
    backward  g[n, c, k] = d_mean[n, c] / 4 + d_std[n, c] (y4[n, c, k] - y_mean[n, c]) / (3 y_std[n, c])
              dW[4c + k, :] = sum_n g[n, c, k] y[n, :],   db[4c + k] = sum_n g[n, c, k]

EXACT TIER.  With integer y, W, b every y4 is an integer, the mean a multiple of 1/4, every squared deviation a multiple of 1/16: all
below 2^24 in their unit, so fp32 gives them exactly in any order, with or without FMA contraction, and the kernels must agree bit for
bit.  y_std is behind a multiplication by fl(1/3), an addition of eps (which may be contracted into it) and a sqrtf: the
argument of the root carries at most 2.5 e relative (fl(1/3), the product, the sum), the root halves that and adds its own rounding,
under 1 ulp in all; asserted as 4 ulp of sqrt(S / 3 + eps) in float64 (S the exact sum of squared deviations, eps the fp32 value the
ABI passes), which leaves room for a sqrtf that is not correctly rounded.  Channels whose four rows of W and b are equal have
S = 0: y_std = sqrt(eps).  The backward takes y4, y_std, y_mean, d_std, d_mean as inputs, so the cases supply them:
    (a) d_std = 0, d_mean multiples of 4: g is an integer whatever y4, y_std, y_mean hold;
    (b) y_std = 1, d_std a multiple of 3, y4 and y_mean integers: d_std (y4 - y_mean) / 3 is an exact quotient, g an integer per k.
dW and db are then integer sums of integer products: exact in any order, any split over the eight sample lanes, any shuffle tree; with
accumulate = 1 on top of integers as well.  Every builder asserts the premise (`_exact`).

TOLERANCE TIER (Gaussian data).  Reference: float64 autograd of F.linear -> view(N, C, 4) -> var / mean (`autograd64`).  The bounds are
the standard running error bounds from the reference's own operands, e = 2^-24; a length-L fp32 dot product in any order is within
(L + 2) e sum|x_k y_k|.  Forward:
    y4_k      E4 = (nc + 2) e (|b| + |y| |W|^T)
    mean      Em = sum_k E4_k / 4 + 4 e sum_k |y4_k| / 4
    d_k = y4_k - mean                     Ed = E4_k + Em + e |d_k|
    S = sum_k d_k^2                       ES = T + 5 e (S + T),  T = sum_k (2 |d_k| Ed_k + Ed_k^2)
    x = S / 3 + eps                       Ex = ES / 3 + 3 e (x + ES / 3)
    std = sqrt(x)                         Estd = Ex / std + 2 e std           (sqrt(x) - sqrt(x - t) <= t / sqrt(x))
Backward, on the y4 / std / mean the forward kernel saved (within E4 / Estd / Em of the reference):
    d_k again                             Dd = E4_k + Em + e (|d_k| + E4_k + Em)
    den = 3 std                           relative Rd = Estd / (std - Estd) + 2 e
    num = d_std d_k                       En = |d_std| Dd + e |d_std| (|d_k| + Dd)
    q = num / den                         Eq = (En / (3 std (1 - Rd)) + |q| Rd / (1 - Rd)) (1 + e) + e |q|
    g = d_mean / 4 + q                    Eg = Eq + 2 e (|d_mean| / 4 + |q| + Eq)
    dW = g^T y                            sum_n Eg |y| + (N + 2) e sum_n (|g| + Eg) |y|;    db the same with y = 1
No constant comes from the kernels' output; every check reports observed / bound."""
import numpy as np

from _sn_ref import E, _bounded, _exact, _same, _sum32, ulp32   # noqa: F401  (one set of helpers for both oracles)


def forward64(y, w, b, eps):
    y, w = np.asarray(y, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n, c = y.shape[0], w.shape[0] // 4
    y4 = y @ w.T
    if b is not None:
        y4 = y4 + np.asarray(b, dtype=np.float64)
    y4 = y4.reshape(n, c, 4)
    mean = y4.sum(-1) / 4
    S = ((y4 - mean[..., None]) ** 2).sum(-1)
    return dict(y4=y4, y_mean=mean, S=S, y_std=np.sqrt(S / 3 + float(np.float32(eps))))


def backward64(d_std, d_mean, y, y4, y_std, y_mean):
    d_std, d_mean, y, y4, y_std, y_mean = (np.asarray(t, dtype=np.float64) for t in (d_std, d_mean, y, y4, y_std, y_mean))
    n, c = d_std.shape
    g = d_mean[..., None] / 4 + d_std[..., None] * (y4.reshape(n, c, 4) - y_mean[..., None]) / (3 * y_std[..., None])
    g = g.reshape(n, 4 * c)
    return dict(g=g, dw=g.T @ y, db=g.sum(0))


def autograd64(y, w, b, eps, d_std, d_mean):
    """float64 autograd of the stock formulation: (y_std, y_mean, dW, db)."""
    import torch
    import torch.nn.functional as F
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    wt = t64(w).clone().requires_grad_(True)
    bt = t64(b).clone().requires_grad_(True) if b is not None else None
    y_ = F.linear(t64(y), wt, bt).view(y.shape[0], -1, 4)
    std = (y_.var(dim=-1) + float(np.float32(eps))).sqrt()
    mean = y_.mean(dim=-1)
    (std * t64(d_std)).sum().add((mean * t64(d_mean)).sum()).backward()
    return dict(y_std=std.detach().numpy(), y_mean=mean.detach().numpy(), dw=wt.grad.numpy(), db=bt.grad.numpy() if bt is not None else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier
# ---------------------------------------------------------------------------------------------------------------------------------
def int_y(N, nc, seed):
    """The integer conditioning input (the levels of a _multi call share one)."""
    return np.random.default_rng(seed).integers(-3, 4, (N, nc)).astype(np.int64)


def fwd_case(N, C, nc, seed, bias=True, eps=1e-5, y=None):
    rng = np.random.default_rng(seed)
    y = int_y(N, nc, seed + 1) if y is None else y
    w = rng.integers(-3, 4, (4 * C, nc)).astype(np.int64)
    b = rng.integers(-5, 6, 4 * C).astype(np.int64) if bias else None
    flat = [c for c in range(C) if c % 3 == 0]                          # channels with four equal values: std = sqrt(eps)
    for c in flat:
        w[4 * c:4 * c + 4] = w[4 * c]
        if bias:
            b[4 * c:4 * c + 4] = b[4 * c]
    _exact(int(np.max(np.abs(y) @ np.abs(w).T + (np.abs(b) if bias else 0))), "y4")
    ref = forward64(y, w, b, eps)
    _exact(int(np.max(ref["S"]) * 16) + 16 * int(np.max(np.abs(ref["y4"]))) * 4, "squared deviations")
    assert np.all(ref["S"][:, flat] == 0) and np.all(ref["y_std"][:, flat] == np.sqrt(float(np.float32(eps))))
    f32 = lambda a: None if a is None else a.astype(np.float32)         # noqa: E731
    return dict(N=N, C=C, nc=nc, eps=eps, y=f32(y), w=f32(w), b=f32(b), flat=flat, y4=f32(ref["y4"]), y_mean=f32(ref["y_mean"]),
                y_std=ref["y_std"])


def check_fwd(case, got, what=""):
    """got: y_std, y_mean (N, C) and optionally y4 (N, C, 4), fp32."""
    tag = f"{what} style fwd N{case['N']} C{case['C']} nc{case['nc']}"
    _same(f"{tag}: y_mean", got["y_mean"], case["y_mean"])
    if got.get("y4") is not None:
        _same(f"{tag}: y4", got["y4"], case["y4"])
    s = np.asarray(got["y_std"])
    assert s.dtype == np.float32 and s.shape == case["y_std"].shape and not np.isnan(s).any(), f"{tag}: y_std"
    ulps = np.abs(s.astype(np.float64) - case["y_std"]) / np.spacing(case["y_std"].astype(np.float32)).astype(np.float64)
    _bounded(f"{tag}: y_std (ulp of sqrt(S/3 + eps))", ulps.max(), 4.0)


def bwd_case(N, C, nc, seed, tier, y=None):
    """tier 'a': d_std = 0, d_mean multiples of 4, anything finite in y4 / y_std / y_mean;  tier 'b': y_std = 1, d_std multiples of 3."""
    rng = np.random.default_rng(seed)
    y = int_y(N, nc, seed + 1) if y is None else y
    d_mean = 4 * rng.integers(-3, 4, (N, C)).astype(np.int64)
    y4 = rng.integers(-4, 5, (N, C, 4)).astype(np.float64)
    y_mean = rng.integers(-2, 3, (N, C)).astype(np.float64)
    if tier == "a":
        d_std = np.zeros((N, C), dtype=np.int64)
        y_std = rng.choice([0.5, 1.0, 2.0, 3.0], (N, C))
        y4 = y4 + 0.375
    else:
        assert tier == "b"
        d_std = 3 * rng.integers(-2, 3, (N, C)).astype(np.int64)
        y_std = np.ones((N, C))
    ref = backward64(d_std, d_mean, y, y4, y_std, y_mean)
    assert np.all(ref["g"] == np.round(ref["g"])), "g is not an integer"
    _exact(int(np.max(np.abs(d_std)[..., None] * np.abs(y4 - y_mean[..., None]))) if tier == "b" else 0, "d_std (y4 - mean)")
    _exact(int(np.max(np.abs(ref["g"]).T @ np.abs(y))) + 1000, "dW (plus the accumulate base)")
    _exact(int(np.max(np.abs(ref["g"]).sum(0))) + 1000, "db (plus the accumulate base)")
    dw0 = rng.integers(-1000, 1001, (4 * C, nc))
    db0 = rng.integers(-1000, 1001, 4 * C)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                     # noqa: E731
    return dict(N=N, C=C, nc=nc, tier=tier, y=f32(y), d_std=f32(d_std), d_mean=f32(d_mean), y4=f32(y4), y_std=f32(y_std), y_mean=f32(y_mean),
                dw=f32(ref["dw"]), db=f32(ref["db"]), dw0=f32(dw0), db0=f32(db0), dw_acc=f32(ref["dw"] + dw0), db_acc=f32(ref["db"] + db0))


def check_bwd(case, dw, db, accumulate, what=""):
    tag = f"{what} style bwd({case['tier']}) N{case['N']} C{case['C']} nc{case['nc']} accumulate {accumulate}"
    _same(f"{tag}: dW", dw, case["dw_acc" if accumulate else "dw"])
    if db is not None:
        _same(f"{tag}: db", db, case["db_acc" if accumulate else "db"])


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 evaluation in a random summation order (tests/test_style_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def forward32(y, w, b, eps, rng):
    y, w = np.asarray(y, dtype=np.float32), np.asarray(w, dtype=np.float32)
    n, c = y.shape[0], w.shape[0] // 4
    terms = y[:, None, :] * w[None, :, :]
    if b is not None:
        terms = np.concatenate([terms, np.broadcast_to(np.asarray(b, dtype=np.float32)[None, :, None], (n, 4 * c, 1))], axis=2)
    y4 = _sum32(terms, 2, rng).reshape(n, c, 4)
    mean = _sum32(y4, 2, rng) * np.float32(0.25)
    d = y4 - mean[..., None]
    var = _sum32(d * d, 2, rng) * (np.float32(1) / np.float32(3))
    return dict(y4=y4, y_mean=mean, y_std=np.sqrt(var + np.float32(eps)))


def backward32(d_std, d_mean, y, y4, y_std, y_mean, rng):
    d_std, d_mean, y, y4, y_std, y_mean = (np.asarray(t, dtype=np.float32) for t in (d_std, d_mean, y, y4, y_std, y_mean))
    n, c = d_std.shape
    g = d_mean[..., None] * np.float32(0.25) + d_std[..., None] * (y4 - y_mean[..., None]) / (np.float32(3) * y_std[..., None])
    g = g.reshape(n, 4 * c)
    return dict(dw=_sum32(g[:, :, None] * y[:, None, :], 0, rng), db=_sum32(g, 0, rng))


# ---------------------------------------------------------------------------------------------------------------------------------
# tolerance tier
# ---------------------------------------------------------------------------------------------------------------------------------
def tolerance_bounds(y, w, b, eps, d_std, d_mean):
    """Elementwise bounds (module docstring) of y_std, y_mean, dW, db for fp32 inputs y, w, b and output gradients d_std, d_mean."""
    y, w, d_std, d_mean = (np.asarray(t, dtype=np.float64) for t in (y, w, d_std, d_mean))
    n, nc = y.shape
    c = w.shape[0] // 4
    ref = forward64(y, w, b, eps)
    y4, mean, S, std = ref["y4"], ref["y_mean"], ref["S"], ref["y_std"]
    E4 = ((nc + 2) * E * (np.abs(y) @ np.abs(w).T + (np.abs(np.asarray(b, dtype=np.float64)) if b is not None else 0))).reshape(n, c, 4)
    Em = E4.sum(-1) / 4 + 4 * E * np.abs(y4).sum(-1) / 4
    d = y4 - mean[..., None]
    Ed = E4 + Em[..., None] + E * np.abs(d)
    T = (2 * np.abs(d) * Ed + Ed ** 2).sum(-1)
    ES = T + 5 * E * (S + T)
    x = S / 3 + float(np.float32(eps))
    Ex = ES / 3 + 3 * E * (x + ES / 3)
    Estd = Ex / std + 2 * E * std
    assert np.all(Estd < std / 2)
    Dd = E4 + Em[..., None] + E * (np.abs(d) + E4 + Em[..., None])
    Rd = (Estd / (std - Estd) + 2 * E)[..., None]
    ads = np.abs(d_std)[..., None]
    En = ads * Dd + E * ads * (np.abs(d) + Dd)
    q = np.abs(d_std[..., None] * d / (3 * std[..., None]))
    Eq = (En / (3 * std[..., None] * (1 - Rd)) + q * Rd / (1 - Rd)) * (1 + E) + E * q
    Eg = (Eq + 2 * E * (np.abs(d_mean)[..., None] / 4 + q + Eq)).reshape(n, 4 * c)
    g = np.abs(backward64(d_std, d_mean, y, y4, std, mean)["g"])
    ay = np.abs(y)
    return dict(y_std=Estd, y_mean=Em, dw=Eg.T @ ay + (n + 2) * E * ((g + Eg).T @ ay), db=Eg.sum(0) + (n + 2) * E * (g + Eg).sum(0))


def check_tolerance(what, ref, bounds, got):
    """ref: autograd64(); got: fp32 arrays under the same keys (db may be None on both sides).  Returns the worst observed / bound."""
    worst = 0.0
    for key in ("y_std", "y_mean", "dw", "db"):
        if ref.get(key) is None:
            assert got.get(key) is None
            continue
        g = np.asarray(got[key], dtype=np.float64)
        assert g.shape == ref[key].shape and not np.isnan(g).any(), f"{what}: {key} shape / NaN"
        ratio = np.abs(g - ref[key]) / bounds[key]
        i = int(np.argmax(ratio))
        worst = max(worst, _bounded(f"{what}: {key} (worst element, flat index {i})", np.abs(g - ref[key]).reshape(-1)[i],
                                    bounds[key].reshape(-1)[i]))
    return worst
