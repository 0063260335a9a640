"""CPU oracles for csrc/spectral_norm.hip (wu_spectral_norm_{fwd,bwd} and their _multi forms).  numpy / torch only, nothing from wu.

    forward   v <- a / max(|a|, eps), a = W^T u;   u <- b / max(|b|, eps), b = W v;   sigma = u . b;   W_eff = W / sigma
              (power_iter = 0: u, v stay, sigma = u . (W v))
    backward  dW = G / sigma - (<G, W> / sigma^2) u v^T            (u, v constants of the graph, as in torch.nn.utils.spectral_norm)

EXACT TIER.  The builders choose data for which every signed sum the kernels form is an integer or a dyadic rational below 2^24 in its
own unit.  fp32 addition of such values is exact in any order, with or without FMA contraction, so whatever the row groups, column blocks,
trees and grid caps, the kernels must agree with the oracle BIT FOR BIT.  Every builder asserts that premise (`_exact`).  The trick that
carries exactness through the first normalisation: four reserved columns of W, spread over the column range, hold one entry each (in
row r = the last row of the first 32-row group, u[r] = 1), set by a four-square decomposition so that |W^T u|^2 = 4^m, with m chosen so
that they carry a fifth of that sum at least (losing row r or a reserved column moves every pinned quantity); then |a| = 2^m,
v = a 2^-m is dyadic and b = W v is exact again.  u is non-zero at both edges of every row group.  Only quantities
behind a sum of positive non-dyadic terms, a sqrtf or a division carry a bound, and that bound is derived, with e = 2^-24 (the fp32 unit
round-off):

    tot = sum_i b_i^2 in any order           relative error <= rows e   (one rounding per square, rows - 1 per addition, first order)
    sigma = tot * (1 / sqrt(tot))            the SAME tot under the root: rows e / 2, plus sqrt, reciprocal and product: 3 e
    u_i = b_i * (1 / sqrt(tot))              b_i exact: rows e / 2 + 3 e
  asserted as |x - x64| <= (rows + 8) e |x64|, which covers the above with the second-order terms (rows <= 513: rows^2 e^2 < 2^-30);
  1 / sigma and W_eff = W * (1 / sigma) take one resp. two more roundings: the same bound plus 2 ulp (4 e).
A dropped or doubled row or column moves these quantities by about 1 / rows or more: tests/test_sn_ref_cpu.py plants such faults.

TOLERANCE TIER (Gaussian data).  Reference: stock torch.nn.utils.spectral_norm in float64 (`StockSN`), fed per call with exactly the
fp32 inputs the kernels get, so no input error enters.  The bound of each quantity is the standard running error bound, evaluated in
float64 from the reference's own operands.  A length-L fp32 dot product in any order: |fl(x . y) - x . y| <= (L + 2) e sum|x_k y_k|
(gamma_L = L e / (1 - L e) <= (L + 2) e for L e < 1/8).  With |M| the elementwise absolute value, s = |W|_2, sa = | |W| |_2:

    a = W^T u    Ea = (rows + 2) e | |W|^T |u| |_2                                    (2-norm of the per-column bounds)
    v = a / |a|  Ev = Ea / (|a| - Ea) + (cols / 2 + 8) e      Dunkl-Williams: |x/|x| - y/|y|| <= 2 |x - y| / (|x| + |y|); the fp32
                                                              norm has relative error (cols + 2) e / 2 + e, the reciprocal and the product
                                                              one e each, rounded up to (cols / 2 + 8) e
    b = W v      Eb = (cols + 2) e (| |W| |v| |_2 + sa Ev) + s Ev                     (rounding on the perturbed v, plus W applied to it)
    u = b / |b|  Eu = Eb / (|b| - Eb) + (rows / 2 + 8) e
    sigma = |b|  Es = Eb + (rows / 2 + 8) e (|b| + Eb)
    1 / sigma    relative Ri = Es / (sigma - Es) + 2 e
    W_eff        elementwise |W_ij| / sigma * (Ri + 2 e)
  power_iter = 0 (u, v are inputs, exact):
    b = W v      Eb = (cols + 2) e | |W| |v| |_2
    sigma = u.b  Es = (rows + 2) e |u| . (|b| + Eb) + |u|_2 Eb
  backward (u, v: the saved copies, within Eu / Ev of the reference's NORM-wise, hence each element too; sigma within Ri):
    d = <G, W>   Ed = (rows cols + 2) e sum |G_ij W_ij|
    c = d / sigma^2          Ec = Ed / sigma^2 (1 + 3 Ri) + |c| (2 Ri + Ri^2 + 3 e)
    dW_ij        |G_ij| / sigma (Ri + 2 e) + Ec (|u_i| + Eu)(|v_j| + Ev) + |c| (Eu |v_j| + |u_i| Ev + Eu Ev)
                 + 3 e (|c| (|u_i| + Eu)(|v_j| + Ev) + |G_ij| / sigma)
  No constant comes from the kernels' output; every check reports observed / bound."""
import math

import numpy as np

E = 2.0 ** -24
LIMIT = 2 ** 24

# rows x cols of the exact power-iteration tier (tests/test_gpu_spectral_norm.py says what each exercises)
POWER_SHAPES = [(1, 5), (1, 512), (3, 27), (2, 6), (31, 255), (32, 256), (33, 257), (64, 27), (70, 600), (257, 40), (260, 300),
                (129, 1153), (257, 1025), (513, 1025)]
NARROW_SHAPES = [(4, 1), (9, 3)]           # fewer than 5 columns: no room for the four reserved ones


def _exact(bound, what):
    """The premise of the exact tier: every partial sum is an integer (in its unit) below 2^24."""
    assert bound < LIMIT, f"exact oracle out of range ({what}): worst-case sum {bound} >= 2^24"


def _bounded(what, err, bound):
    """Assert err <= bound and report observed / bound (printed, and in the message)."""
    err, bound = float(err), float(bound)
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{what}: observed {err:.3e} / bound {bound:.3e} = {ratio:.3f}")
    assert err <= bound, f"{what}: observed {err:.3e} / bound {bound:.3e} = {ratio:.3f}"
    return ratio


def _same(what, got, want):
    """Equality of values (NaN anywhere fails; +0 and -0 compare equal)."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ from the exact oracle; first at flat index {i} "
                             f"(got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}), last at {int(bad[-1])}")


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def four_squares(d):
    """(a, b, c, e) with a^2 + b^2 + c^2 + e^2 = d (Lagrange), largest first."""
    assert d >= 0
    for a in range(math.isqrt(d), -1, -1):
        r1 = d - a * a
        for b in range(min(a, math.isqrt(r1)), -1, -1):
            r2 = r1 - b * b
            for c in range(min(b, math.isqrt(r2)), -1, -1):
                r3 = r2 - c * c
                e = math.isqrt(r3)
                if e * e == r3 and e <= c:
                    return a, b, c, e
    raise AssertionError(d)


def reserved_columns(cols):
    """Four distinct columns spread over the range (one per quarter, mid-quarter)."""
    assert cols >= 5
    res = [k * cols // 4 + cols // 8 for k in range(4)]
    assert len(set(res)) == 4 and res[-1] < cols
    return res


def _sparse_w(rng, rows, cols):
    return rng.integers(-2, 3, (rows, cols)) * (rng.random((rows, cols)) < 0.15)


# ---------------------------------------------------------------------------------------------------------------------------------
# closed forms in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def forward64(W, u, v, power_iter, eps):
    """The operation in float64 (eps as the fp32 value the ABI passes)."""
    W, u, v = (np.asarray(t, dtype=np.float64) for t in (W, u, v))
    eps = float(np.float32(eps))
    out = {}
    if power_iter:
        a = W.T @ u
        v = a / max(np.linalg.norm(a), eps)
        b = W @ v
        u = b / max(np.linalg.norm(b), eps)
        out.update(v_raw=a)
    else:
        b = W @ v
    sigma = float(u @ b)
    with np.errstate(divide="ignore", invalid="ignore"):
        out.update(u=u, v=v, u_raw=b, sigma=sigma, w_eff=W / sigma)
    return out


def backward64(G, W, u, v, sigma):
    G, W, u, v = (np.asarray(t, dtype=np.float64) for t in (G, W, u, v))
    return G / sigma - (np.sum(G * W) / sigma ** 2) * np.outer(u, v)


class StockSN:
    """Stock torch.nn.utils.spectral_norm in float64 around a bare weight: the independent reference of the tolerance tier."""

    def __init__(self, W, eps):
        import torch

        class Bare(torch.nn.Module):
            def __init__(self, w):
                super().__init__()
                self.weight = torch.nn.Parameter(w)

            def forward(self):
                return self.weight

        self.torch = torch
        self.mod = torch.nn.utils.spectral_norm(Bare(torch.as_tensor(np.asarray(W), dtype=torch.float64).clone()), n_power_iterations=1,
                                                eps=float(np.float32(eps)))

    def step(self, u, v, train, G=None):
        """One forward from the buffers (u, v) (and a backward of G): dict of float64 arrays."""
        torch = self.torch
        self.mod.train(train)
        with torch.no_grad():
            self.mod.weight_u.copy_(torch.as_tensor(np.asarray(u), dtype=torch.float64))
            self.mod.weight_v.copy_(torch.as_tensor(np.asarray(v), dtype=torch.float64))
        self.mod.weight_orig.grad = None
        w_eff = self.mod()
        out = dict(w_eff=w_eff.detach().numpy().copy(), u=self.mod.weight_u.numpy().copy(), v=self.mod.weight_v.numpy().copy())
        if G is not None:
            w_eff.backward(torch.as_tensor(np.asarray(G), dtype=torch.float64))
            out["dw"] = self.mod.weight_orig.grad.numpy().copy()
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier: power iteration
# ---------------------------------------------------------------------------------------------------------------------------------
def power_case(rows, cols, seed):
    """Integer W (entries in [-2, 2], ~15 % dense, plus the four reserved entries), u in {-1, 0, 1}: |W^T u| = 2^m."""
    rng = np.random.default_rng(seed)
    W = _sparse_w(rng, rows, cols).astype(np.int64)
    u = rng.integers(-1, 2, rows).astype(np.int64)
    edge = [i for i in range(rows) if i % 32 in (0, 31) or i == rows - 1]      # the rows at the edges of a 32-row group always count
    u[edge] = rng.choice([-1, 1], len(edge))
    r = min(31, rows - 1)                       # the reserved entries sit in the LAST row of the first row group
    u[r] = 1
    res = reserved_columns(cols)
    W[:, res] = 0
    n2 = int(np.sum((W.T @ u) ** 2))
    m = 0
    while 4 * 4 ** m < 5 * max(n2, 1):          # the reserved columns carry a fifth of |W^T u|^2 at least: losing row r moves sigma too
        m += 1
    sq = list(four_squares(4 ** m - n2))
    sq = [sq[i] for i in rng.permutation(4)]
    W[r, res] = np.array(sq) * rng.choice([-1, 1], 4)
    v_raw = W.T @ u
    assert int(np.sum(v_raw ** 2)) == 4 ** m
    _exact(int(np.max(np.abs(W).T @ np.abs(u))), "W^T u")
    _exact(4 ** m - 1, "|W^T u|^2")                                   # 4^m itself is a power of two: representable
    u_raw_int = W @ v_raw                                              # in units of 2^-m
    _exact(int(np.max(np.abs(W) @ np.abs(v_raw))), "W v")
    tot = sum(int(x) ** 2 for x in u_raw_int)
    assert tot > 0, "degenerate case: W v = 0"
    sigma = math.sqrt(tot) / 2 ** m
    return dict(rows=rows, cols=cols, W=W.astype(np.float32), u=u.astype(np.float32), v0=rng.standard_normal(cols).astype(np.float32),
                r=r, m=m, reserved=res, v_raw=v_raw.astype(np.float32), v=(v_raw / 2.0 ** m).astype(np.float32),
                u_raw=(u_raw_int / 2.0 ** m).astype(np.float32), sigma=sigma, u_new=(u_raw_int / 2.0 ** m) / sigma,
                tot_units=tot, eps=1e-12)


def check_power(case, got, what=""):
    """got: dict of fp32 arrays the kernels produced: v, u, sigma (2) and optionally v_save, u_save, w_eff, v_raw, u_raw."""
    tag = f"{what} power {case['rows']}x{case['cols']}"
    _same(f"{tag}: v", got["v"], case["v"])
    if got.get("v_save") is not None:
        _same(f"{tag}: v_save", got["v_save"], case["v"])
    if got.get("v_raw") is not None:
        _same(f"{tag}: W^T u (scratch)", got["v_raw"], case["v_raw"])
    if got.get("u_raw") is not None:
        _same(f"{tag}: W v (scratch)", got["u_raw"], case["u_raw"])
    rel = (case["rows"] + 8) * E
    s64 = case["sigma"]
    sigma = np.asarray(got["sigma"], dtype=np.float64)
    _bounded(f"{tag}: sigma", abs(sigma[0] - s64), rel * s64)
    _bounded(f"{tag}: 1/sigma", abs(sigma[1] - 1 / s64), (rel + 4 * E) / s64)
    un = case["u_new"]
    for key in ("u", "u_save"):
        if got.get(key) is not None:
            g = np.asarray(got[key], dtype=np.float64)
            assert g.shape == un.shape and not np.isnan(g).any(), f"{tag}: {key} has NaN"
            zero = un == 0
            assert np.all(g[zero] == 0), f"{tag}: {key} non-zero where W v = 0"
            _bounded(f"{tag}: {key} (u_raw / sigma, worst element relative)", np.max(np.abs(g - un)[~zero] / np.abs(un[~zero])), rel)
    if got.get("u_save") is not None:
        _same(f"{tag}: u_save is the u written", got["u_save"], got["u"])
    if got.get("w_eff") is not None:
        w = np.asarray(got["w_eff"], dtype=np.float64)
        W = case["W"].astype(np.float64)
        assert w.shape == W.shape and not np.isnan(w).any(), f"{tag}: w_eff has NaN"
        nz = W != 0
        assert np.all(w[~nz] == 0), f"{tag}: w_eff non-zero where W = 0"
        _bounded(f"{tag}: w_eff (worst element relative)", np.max(np.abs(w - W / s64)[nz] / np.abs(W[nz] / s64)), rel + 4 * E)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier: power_iter = 0
# ---------------------------------------------------------------------------------------------------------------------------------
def iter0_case(rows, cols, seed):
    """Integer W, u, v in [-2, 2]: sigma = u . (W v) is an exact non-zero integer."""
    for t in range(100):
        rng = np.random.default_rng(seed + 1000 * t)
        W = rng.integers(-2, 3, (rows, cols)).astype(np.int64)
        u = rng.integers(-2, 3, rows).astype(np.int64)
        v = rng.integers(-2, 3, cols).astype(np.int64)
        b = W @ v
        sigma = int(u @ b)
        if sigma != 0:
            break
    assert sigma != 0
    _exact(int(np.max(np.abs(W) @ np.abs(v))), "W v")
    _exact(int(np.abs(u) @ np.abs(b)), "u . (W v)")
    return dict(rows=rows, cols=cols, W=W.astype(np.float32), u=u.astype(np.float32), v=v.astype(np.float32), u_raw=b.astype(np.float32),
                sigma=float(sigma), eps=1e-12)


def check_iter0(case, got, what=""):
    """got: u, v (the buffers after the call), sigma (2), optionally u_save, v_save, w_eff, u_raw."""
    tag = f"{what} iter0 {case['rows']}x{case['cols']}"
    _same(f"{tag}: u untouched", got["u"], case["u"])
    _same(f"{tag}: v untouched", got["v"], case["v"])
    for key, src in (("u_save", "u"), ("v_save", "v")):
        if got.get(key) is not None:
            _same(f"{tag}: {key} is a copy", got[key], case[src])
    if got.get("u_raw") is not None:
        _same(f"{tag}: W v (scratch)", got["u_raw"], case["u_raw"])
    sigma = np.asarray(got["sigma"])
    _same(f"{tag}: sigma", sigma[:1], np.array([case["sigma"]]))
    _bounded(f"{tag}: 1/sigma", abs(float(sigma[1]) - 1.0 / case["sigma"]), ulp32(1.0 / case["sigma"]))
    if got.get("w_eff") is not None:
        _same(f"{tag}: w_eff = fl(W * sigma_out[1])", got["w_eff"], case["W"] * np.float32(sigma[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier: the eps clamp
# ---------------------------------------------------------------------------------------------------------------------------------
def clamp_case(rows, cols, seed, k, s):
    """eps = 2^k, u = integers * 2^-s with |W^T u| < eps / 2: v = (W^T u) / eps exactly.  `u_clamped` says on which side of eps
    |W v| falls (a factor 2 away from it at least): clamped, u = (W v) / eps exactly as well."""
    rng = np.random.default_rng(seed)
    W = _sparse_w(rng, rows, cols).astype(np.int64)
    W[rng.integers(rows), :] = rng.integers(-2, 3, cols)               # one dense row: small shapes are not all zero
    u = rng.integers(-1, 2, rows).astype(np.int64)
    u[int(rng.integers(rows))] = 1
    a = W.T @ u                                                         # units of 2^-s
    _exact(int(np.max(np.abs(W).T @ np.abs(u))), "W^T u")
    n2 = sum(int(x) ** 2 for x in a)
    _exact(n2, "|W^T u|^2")
    assert n2 > 0 and 4 * n2 < 4 ** (k + s), f"|W^T u| = {math.sqrt(n2)} 2^-{s} is not below eps / 2 = 2^{k - 1}"
    b = W @ a                                                           # units of 2^-(s + k)
    _exact(int(np.max(np.abs(W) @ np.abs(a))), "W v")
    tot = sum(int(x) ** 2 for x in b)                                   # units of 4^-(s + k)
    assert tot > 0
    assert 2 * k + s >= 0
    lim = 4 ** (2 * k + s)                                              # eps^2 in the same units
    u_clamped = 4 * tot < lim
    assert u_clamped or tot > 4 * lim, "|W v| within a factor 2 of eps: choose another k / s"
    unit = 2.0 ** -(s + k)
    nb = math.sqrt(tot) * unit
    den = 2.0 ** k if u_clamped else nb
    return dict(rows=rows, cols=cols, W=W.astype(np.float32), u=(u * 2.0 ** -s).astype(np.float32),
                v0=rng.standard_normal(cols).astype(np.float32), eps=2.0 ** k, v=(a * unit).astype(np.float32),
                u_raw=(b * unit).astype(np.float32), u_clamped=u_clamped, u_new=b * unit / den, sigma=nb * nb / den)


def check_clamp(case, got, what=""):
    tag = f"{what} clamp {case['rows']}x{case['cols']} eps {case['eps']}"
    _same(f"{tag}: v = W^T u / eps", got["v"], case["v"])
    if got.get("v_save") is not None:
        _same(f"{tag}: v_save", got["v_save"], case["v"])
    if got.get("u_raw") is not None:
        _same(f"{tag}: W v (scratch)", got["u_raw"], case["u_raw"])
    rel = (case["rows"] + 8) * E
    un = case["u_new"]
    for key in ("u", "u_save"):
        if got.get(key) is None:
            continue
        if case["u_clamped"]:
            _same(f"{tag}: {key} = W v / eps", got[key], un)
        else:
            g = np.asarray(got[key], dtype=np.float64)
            nz = un != 0
            assert not np.isnan(g).any() and np.all(g[~nz] == 0)
            _bounded(f"{tag}: {key} (worst element relative)", np.max(np.abs(g - un)[nz] / np.abs(un[nz])), rel)
    sigma = np.asarray(got["sigma"], dtype=np.float64)
    s64 = case["sigma"]
    _bounded(f"{tag}: sigma", abs(sigma[0] - s64), rel * s64)
    _bounded(f"{tag}: 1/sigma", abs(sigma[1] - 1 / s64), (rel + 4 * E) / s64)
    if got.get("w_eff") is not None:
        w = np.asarray(got["w_eff"], dtype=np.float64)
        W = case["W"].astype(np.float64)
        nz = W != 0
        assert not np.isnan(w).any() and np.all(w[~nz] == 0)
        _bounded(f"{tag}: w_eff (worst element relative)", np.max(np.abs(w - W / s64)[nz] / np.abs(W[nz] / s64)), rel + 4 * E)


def check_zero(rows, cols, got, what=""):
    """All-zero W: sigma = 0 and W_eff = 0 / 0 = NaN everywhere -- what torch.nn.utils.spectral_norm gives; u, v become zero."""
    tag = f"{what} zero W {rows}x{cols}"
    _same(f"{tag}: v", got["v"], np.zeros(cols))
    _same(f"{tag}: u", got["u"], np.zeros(rows))
    sigma = np.asarray(got["sigma"])
    assert sigma[0] == 0 and np.isposinf(sigma[1]), f"{tag}: sigma pair {sigma}"
    assert np.isnan(np.asarray(got["w_eff"])).all() and np.asarray(got["w_eff"]).shape == (rows, cols), f"{tag}: w_eff is not all NaN"


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier: backward
# ---------------------------------------------------------------------------------------------------------------------------------
def bwd_case(rows, cols, seed, a):
    """Integer G in [-3, 3], W in [-2, 2], u, v in quarters, sigma = (2^a, 2^-a): <G, W> and every dW element are exact dyadics."""
    rng = np.random.default_rng(seed)
    G = rng.integers(-3, 4, (rows, cols)).astype(np.int64)
    W = rng.integers(-2, 3, (rows, cols)).astype(np.int64)
    u4 = rng.integers(-4, 5, rows).astype(np.int64)
    v4 = rng.integers(-4, 5, cols).astype(np.int64)
    _exact(int(np.sum(np.abs(G * W))), "<G, W>")
    dot = int(np.sum(G * W))
    _exact(abs(dot) * 4, "c u")
    _exact(abs(dot) * 16, "c u v")
    # dW in units of 2^-(2a + 4):  G 2^(a + 4) - dot u4 v4
    dw_units = G * 2 ** (a + 4) - dot * np.outer(u4, v4)
    assert a >= -4
    _exact(int(np.max(np.abs(G))) * 2 ** (a + 4) + abs(dot) * 16, "dW")
    return dict(rows=rows, cols=cols, G=G.astype(np.float32), W=W.astype(np.float32), u=(u4 / 4.0).astype(np.float32),
                v=(v4 / 4.0).astype(np.float32), sigma=np.array([2.0 ** a, 2.0 ** -a], dtype=np.float32), dot=dot,
                dw=(dw_units * 2.0 ** -(2 * a + 4)).astype(np.float32))


def check_bwd(case, dw, what=""):
    _same(f"{what} backward {case['rows']}x{case['cols']}: dW", dw, case["dw"])


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 evaluation in a random summation order (tests/test_sn_ref_cpu.py: the exact tier does not depend on the order)
# ---------------------------------------------------------------------------------------------------------------------------------
def _sum32(terms, axis, rng):
    """fp32 sum along `axis`, sequential, every line in its own random order."""
    terms = np.asarray(terms, dtype=np.float32)
    order = np.argsort(rng.random(terms.shape), axis=axis)
    return np.take(np.cumsum(np.take_along_axis(terms, order, axis=axis), axis=axis, dtype=np.float32), -1, axis=axis)


def forward32(W, u, v, power_iter, eps, rng):
    """The forward in fp32, every sum in a random order: the arithmetic of the kernels up to the order of additions."""
    W, u, v = (np.asarray(t, dtype=np.float32) for t in (W, u, v))
    eps = np.float32(eps)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        if power_iter:
            a = _sum32(W * u[:, None], 0, rng)
            inv = np.float32(1) / max(np.sqrt(_sum32(a * a, 0, rng)), eps)
            v = a * inv
            out["v_raw"] = a
        b = _sum32(W * v[None, :], 1, rng)
        if power_iter:
            tot = _sum32(b * b, 0, rng)
            inv = np.float32(1) / max(np.sqrt(tot), eps)
            u = b * inv
            sigma = tot * inv
        else:
            sigma = _sum32(u * b, 0, rng)
        s1 = np.float32(1) / sigma
        out.update(u=u, v=v, u_raw=b, sigma=np.array([sigma, s1], dtype=np.float32), w_eff=W * s1)
    return out


def backward32(G, W, u, v, sigma, rng):
    G, W, u, v, sigma = (np.asarray(t, dtype=np.float32) for t in (G, W, u, v, sigma))
    dot = _sum32((G * W).reshape(-1), 0, rng)
    c = dot * sigma[1] * sigma[1]
    return G * sigma[1] - (c * u)[:, None] * v[None, :]


# ---------------------------------------------------------------------------------------------------------------------------------
# tolerance tier: running error bounds from the reference's operands (module docstring)
# ---------------------------------------------------------------------------------------------------------------------------------
def forward_bounds(W, u, v, power_iter):
    """W (fp32 values), u, v: the buffers BEFORE the call.  Returns the bounds of the module docstring and the float64 operands."""
    W, u, v = (np.asarray(t, dtype=np.float64) for t in (W, u, v))
    rows, cols = W.shape
    A = np.abs(W)
    s, sa = np.linalg.norm(W, 2), np.linalg.norm(A, 2)
    if power_iter:
        a = W.T @ u
        na = np.linalg.norm(a)
        Ea = (rows + 2) * E * np.linalg.norm(A.T @ np.abs(u))
        assert Ea < na / 2
        Ev = Ea / (na - Ea) + (cols / 2 + 8) * E
        v = a / na
        b = W @ v
        nb = np.linalg.norm(b)
        Eb = (cols + 2) * E * (np.linalg.norm(A @ np.abs(v)) + sa * Ev) + s * Ev
        assert Eb < nb / 2
        Eu = Eb / (nb - Eb) + (rows / 2 + 8) * E
        u = b / nb
        sigma = nb
        Es = Eb + (rows / 2 + 8) * E * (nb + Eb)
    else:
        b = W @ v
        Eu = Ev = 0.0
        Eb = (cols + 2) * E * np.linalg.norm(A @ np.abs(v))
        sigma = float(u @ b)
        Es = (rows + 2) * E * float(np.abs(u) @ (np.abs(b) + Eb)) + np.linalg.norm(u) * Eb
    assert Es < abs(sigma) / 2
    Ri = Es / (abs(sigma) - Es) + 2 * E
    return dict(u=u, v=v, sigma=sigma, Eu=Eu, Ev=Ev, Es=Es, Ri=Ri, w_eff=A / abs(sigma) * (Ri + 2 * E))


def backward_bounds(G, W, fb):
    """Elementwise bound of dW; fb: forward_bounds() of the forward whose saved u, v, sigma the backward uses."""
    G, W = np.asarray(G, dtype=np.float64), np.asarray(W, dtype=np.float64)
    sigma, Ri, Eu, Ev = abs(fb["sigma"]), fb["Ri"], fb["Eu"], fb["Ev"]
    au, av = np.abs(fb["u"])[:, None], np.abs(fb["v"])[None, :]
    Ed = (G.size + 2) * E * np.sum(np.abs(G * W))
    c = abs(np.sum(G * W)) / sigma ** 2
    Ec = Ed / sigma ** 2 * (1 + 3 * Ri) + c * (2 * Ri + Ri * Ri + 3 * E)
    g = np.abs(G) / sigma
    return (g * (Ri + 2 * E) + Ec * (au + Eu) * (av + Ev) + c * (Eu * av + au * Ev + Eu * Ev)
            + 3 * E * (c * (au + Eu) * (av + Ev) + g))


def check_tolerance(what, ref, fb, got, bwd_bound=None):
    """ref: StockSN.step() output; got: fp32 arrays w_eff, u, v (and dw with bwd_bound).  Returns the worst observed / bound."""
    worst = 0.0
    for key, bound in (("u", fb["Eu"]), ("v", fb["Ev"])):
        g = np.asarray(got[key], dtype=np.float64).reshape(-1)
        assert not np.isnan(g).any(), f"{what}: {key} has NaN"
        if bound == 0:
            assert np.array_equal(g, ref[key]), f"{what}: {key} changed without a power iteration"
        else:
            worst = max(worst, _bounded(f"{what}: |{key} - ref|_2", np.linalg.norm(g - ref[key]), bound))
    pairs = [("w_eff", fb["w_eff"])] + ([("dw", bwd_bound)] if bwd_bound is not None else [])
    for key, bound in pairs:
        g = np.asarray(got[key], dtype=np.float64).reshape(bound.shape)
        assert not np.isnan(g).any(), f"{what}: {key} has NaN"
        err = np.abs(g - ref[key].reshape(bound.shape))
        exact = bound == 0
        assert np.all(err[exact] == 0), f"{what}: {key} wrong where the bound is zero"
        i = np.argmax(np.where(exact, 0, err / np.where(exact, 1, bound)))
        worst = max(worst, _bounded(f"{what}: {key} (worst element, flat index {int(i)})", err.reshape(-1)[i], bound.reshape(-1)[i]))
    return worst
