"""Case tables, operand constructors, bounds and CPU oracles of tests/test_gpu_train_exact.py (no GPU import; checked by
tests/test_train_ref_cpu.py): the kernels that only the TRAINABLE ResNet-101 runs -- train-mode BatchNorm (statistics, apply, backward),
the pointwise and stem weight gradients of csrc/resnet_train.hip, and maxpool3s2 of csrc/resnet.hip.

The library is compiled with the compiler's default FMA contraction, so an fp32 expression with an inexact intermediate has no portable
CPU restatement.  The operands here make every intermediate EXACT instead; then summation order, split count and contraction cannot
change a bit and the float64 value, cast once, is the one right answer:

  BatchNorm   x[r, c] = m_c + a_c s[r, c] with an integer m_c in [-3, 3], a_c in {1/2, 1, 2} and s exactly balanced per channel (half
              -1 / half +1, or 1/8 at -2, 1/8 at +2 and 3/4 at 0): mean m_c and variance a_c^2 exactly, rstd = 1 / a_c a power of two
              at eps = 0; the shifted sums sum (x - K), sum (x - K)^2 of the kernel are multiples of 1/4 that stay below 2^24 quarter
              units.  gamma in {-2, -1, 1/2, 1, 2, 3}, integer beta, integer residual up to 256, integer g in [-4, 4]: the apply output
              and dbeta / dgamma are exact dyadic values for any M, dx for M a power of two (1 / M exact).  For other M dx carries the
              bound of `dx_bound`; running_var carries n / (n - 1) and is held to 2 fp32 ulps.
  weight      integer x and dy, sums below 2^24: torch's CPU fp32 result equals float64.
  gradients
  max-pool    integers in [-2, 2] (most windows tie), +-1/2 in one case; torch's F.max_pool2d and its autograd are the oracle, the
              stored arg-max is restated from the kernel's rule."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from _pointwise_ref import LEAKY, NONE, RELU, SLOPE, TWO24, act_apply, act_gate, ints, unrepresentable  # noqa: F401

TORCH_DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32}
VEC = {"bf16": 8, "fp32": 4}                     # elements per 16-byte vector

# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm: launch arithmetic restated from csrc/resnet_train.hip
# ---------------------------------------------------------------------------------------------------------------------------------
BN_RP = {"bf16": 32, "fp32": 16}                 # rows in flight per workgroup (BnGeom<T>::RP)
BN_MAX_SPLITS = 256                              # kBnMaxSplits
EW_GRID_CAP = 256 * 32                           # ew_grid: workgroups of 256 threads at most


def bn_splits(m, c, dtype):
    """bn_splits of the library: about 1024 workgroups, at least 8 rows per thread, at most kBnMaxSplits."""
    s = (1024 + c // 64 - 1) // (c // 64)
    s = min(s, m // (8 * BN_RP[dtype]), BN_MAX_SPLITS)
    return max(s, 1)


def bn_plan(m, c, dtype):
    """(splits, rows per split, rows of the last split: zero or negative = it starts at or beyond M)."""
    s = bn_splits(m, c, dtype)
    rps = (m + s - 1) // s
    return s, rps, m - (s - 1) * rps


def bn_workspace_floats(m, c, dtype, per_split):
    return bn_splits(m, c, dtype) * per_split * c


GAMMAS = (-2.0, -1.0, 0.5, 1.0, 2.0, 3.0)
SCALES = (0.5, 1.0, 2.0)

# form: "single" | "dual" (x2 with its own m, a, gamma, beta) | "res" (residual);  act: of the apply and the gate of the backward
# (NONE: the backward runs without y);  gres: the backward also writes the gated gradient;  unit: every a_c = 1 (with eps = 3: rstd = 1/2)
# splits / last: the split count and the rows of the last split that the case is in the table FOR ({dtype: (splits, last rows)})
BnCase = collections.namedtuple("BnCase", "name dtypes m c form act gres eps momentum unit seed plan")
BOTH = ("bf16", "fp32")

BN_CASES = [
    # fewer rows than the 32 / 16 in flight
    BnCase("m1", BOTH, 1, 64, "single", RELU, False, 0.25, 0.5, False, 2001, {"bf16": (1, 1), "fp32": (1, 1)}),
    BnCase("m2", BOTH, 2, 64, "res", RELU, True, 0.0, 0.25, False, 2002, {"bf16": (1, 2), "fp32": (1, 2)}),
    BnCase("m30", BOTH, 30, 64, "dual", RELU, True, 0.0, 0.5, False, 2003, {"bf16": (1, 30), "fp32": (1, 30)}),
    # two bf16 splits (four in fp32)
    BnCase("m512", BOTH, 512, 64, "res", RELU, True, 0.0, 0.25, False, 2004, {"bf16": (2, 256), "fp32": (4, 128)}),
    BnCase("m512-eps3", BOTH, 512, 64, "single", NONE, False, 3.0, 0.5, True, 2005, {"bf16": (2, 256), "fp32": (4, 128)}),
    # sixteen even bf16 splits (32 in fp32); C = 192: the blockIdx.x * 64 channel offset and the [split][q][C] partial layout
    BnCase("m4096-c64", BOTH, 4096, 64, "dual", RELU, True, 0.0, 0.5, False, 2006, {"bf16": (16, 256), "fp32": (32, 128)}),
    BnCase("m4096-c192", BOTH, 4096, 192, "res", RELU, True, 0.0, 0.25, False, 2007, {"bf16": (16, 256), "fp32": (32, 128)}),
    BnCase("m4096-leaky", BOTH, 4096, 64, "res", LEAKY, True, 0.0, 0.5, False, 2008, {"bf16": (16, 256), "fp32": (32, 128)}),
    BnCase("m4096-nogate", BOTH, 4096, 64, "single", NONE, False, 0.0, 0.25, False, 2009, {"bf16": (16, 256), "fp32": (32, 128)}),
    # an uneven last split: 16 x 257 rows cover 4112 (bf16), 32 x 129 cover 4128 (fp32)
    BnCase("m4100", BOTH, 4100, 64, "res", RELU, True, 0.0, 0.5, False, 2010, {"bf16": (16, 245), "fp32": (32, 101)}),
    # 256 splits of 129 rows: split 254 keeps 4 rows, split 255 starts at row 32895 > M
    BnCase("m32770-empty-split", ("fp32",), 32770, 64, "single", RELU, False, 0.0, 0.25, False, 2011, {"fp32": (256, -125)}),
    # at and above the 256-split clamp
    BnCase("m65536", BOTH, 65536, 64, "single", RELU, False, 0.0, 0.5, False, 2012, {"bf16": (256, 256), "fp32": (256, 256)}),
    BnCase("m131072", BOTH, 131072, 64, "dual", RELU, True, 0.0, 0.25, False, 2013, {"bf16": (256, 512), "fp32": (256, 512)}),
    # M C / 4 = 2^22 vectors > 256 * 32 * 256: bn_apply_kernel and bn_bwd_dx_kernel walk their grid-stride loop twice
    BnCase("m131072-c128-gridstride", ("fp32",), 131072, 128, "res", RELU, True, 0.0, 0.5, False, 2014, {"fp32": (256, 512)}),
]


BN_BY_NAME = {c.name: c for c in BN_CASES}


def _balanced(m, c, gen, wide):
    """s (M, C): per channel exactly balanced -- half -1 / half +1, or (wide, M % 8 == 0) 1/8 at -2, 1/8 at +2, 3/4 at 0 --, each channel
    in its own random row order.  M = 1: zero."""
    if m == 1:
        return torch.zeros(1, c)
    assert m % 2 == 0
    perm = torch.rand(m, c, generator=gen).argsort(dim=0)          # a permutation of the rows per channel
    r = torch.arange(m)
    two = torch.where(r < m // 2, -1.0, 1.0)[perm]
    if m % 8:
        return two
    three = torch.where(r < m // 8, -2.0, torch.where(r < m // 4, 2.0, 0.0))[perm]
    return torch.where(wide[None, :], three, two)


def _pick(values, c, gen):
    return torch.tensor(values)[torch.randint(0, len(values), (c,), generator=gen)]


def _branch(case, gen):
    """One BatchNorm input with its parameters: x (M, C) fp32 (bf16-representable), design mean m and scale a, gamma, beta."""
    c = case.c
    m = torch.randint(-3, 4, (c,), generator=gen).float()
    a = torch.ones(c) if case.unit else _pick(SCALES, c, gen)
    wide = torch.randint(0, 2, (c,), generator=gen).bool()
    s = _balanced(case.m, c, gen, wide)
    return dict(x=m[None, :] + a[None, :] * s, m=m, a=a, gamma=_pick(GAMMAS, c, gen), beta=torch.randint(-2, 3, (c,), generator=gen).float())


def bn_operands(case):
    """Everything a case feeds its kernels, on the CPU in fp32; every tensor is exact in bf16."""
    gen = torch.Generator().manual_seed(case.seed)
    ops = dict(b1=_branch(case, gen), b2=None, res=None)
    if case.form == "dual":
        ops["b2"] = _branch(case, gen)
    if case.form == "res":
        # small integers (exact zeros before the activation) and, on half of the sites, integers of 128..255 (a quarter of them negative): with the halves of
        # gamma = 1/2 these need nine bits, one more than bf16 has
        small = torch.randint(-3, 4, (case.m, case.c), generator=gen).float()
        big = torch.randint(128, 256, (case.m, case.c), generator=gen).float()
        sign = torch.where(torch.rand(case.m, case.c, generator=gen) < 0.25, -1.0, 1.0)
        ops["res"] = torch.where(torch.rand(case.m, case.c, generator=gen) < 0.5, sign * big, small)
    ops["g"] = torch.randint(-4, 5, (case.m, case.c), generator=gen).float()
    ops["running_mean0"] = torch.randint(-4, 5, (case.c,), generator=gen).float()
    ops["running_var0"] = torch.randint(1, 4, (case.c,), generator=gen).float()
    ops["tracked0"] = 5
    return ops


def stats_bounds(x):
    """Worst-case magnitudes of the kernel's shifted sums over ANY subset of rows, in units of their grid (1/2 for sum (x - K), 1/4 for
    sum (x - K)^2, K = row 0): below 2^24 they are exact in fp32 whatever the order."""
    d = x.double() - x[0].double()[None, :]
    assert bool((d * 2 == (d * 2).round()).all())
    return float((d.abs() * 2).sum(0).max()), float((d * d * 4).sum(0).max())


def bn_stats_reference(case, b):
    """float64 batch statistics: mean, biased variance, rstd = 1 / sqrt(var + eps)."""
    x = b["x"].double()
    mean = x.mean(0)
    var = ((x - mean[None, :]) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + case.eps)


def stats_tensor(mean, rstd):
    """The (2, C) fp32 statistics the kernels exchange; exact by design (asserted)."""
    st = torch.stack([mean, rstd]).float()
    assert torch.equal(st.double(), torch.stack([mean, rstd]))
    return st


def running_reference(case, ops, mean, var):
    """nn.BatchNorm2d's running update: running_mean exact in fp32; running_var in float64 (held to RUNNING_VAR_ULPS)."""
    mom = case.momentum
    rm = mom * mean + (1.0 - mom) * ops["running_mean0"].double()
    n = float(case.m)
    unbiased = var * n / (n - 1.0) if case.m > 1 else var
    rv = mom * unbiased + (1.0 - mom) * ops["running_var0"].double()
    assert torch.equal(rm.float().double(), rm)
    return rm.float(), rv


# running_var = momentum * (float)unbiased + (1 - momentum) * running_var in fp32: the cast of the unbiased variance is off by at most
# half an ulp of it (momentum <= 1/2 scales that below half an ulp of the result, which is at least (1 - momentum) >= 1/2); both products
# are exact (momentum a power of two, running_var a small integer); the sum rounds once, fused or not: half an ulp.  One ulp each, rounded up.
RUNNING_VAR_ULPS = 2


def ulp32(v64):
    """The fp32 ulp at |v| (float64 tensor in, float64 out)."""
    a = v64.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def ulp_bf16(v64):
    a = v64.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _affine64(b, mean, rstd):
    sc = b["gamma"].double() * rstd
    return b["x"].double() * sc[None, :] + (b["beta"].double() - mean * sc)[None, :]


def bn_apply_reference(case, ops, st1, st2):
    """(lin, out): the exact pre-activation value and the activated fp32 value that is rounded ONCE to the storage type.  lin is float64
    arithmetic on dyadic values and must fit fp32 (asserted); LeakyReLU is the kernel's single fp32 multiply by 0.2f."""
    lin = _affine64(ops["b1"], *st1)
    if case.form == "dual":
        lin = lin + _affine64(ops["b2"], *st2)
    elif case.form == "res":
        lin = lin + ops["res"].double()
    lin32 = lin.float()
    assert torch.equal(lin32.double(), lin), "the apply oracle left fp32"
    return lin32, act_apply(lin32, case.act)


def bn_apply_fp32_restatement(case, ops, st1, st2):
    """The kernel's own operation order in fp32 without contraction (sc = gamma rstd; x sc + (beta - mean sc); + second branch or
    residual): on these operands it must equal the float64 oracle."""
    def branch(b, st):
        mean, rstd = st[0].float(), st[1].float()
        sc = b["gamma"] * rstd
        return b["x"] * sc[None, :] + (b["beta"] - mean * sc)[None, :]
    o = branch(ops["b1"], st1)
    if case.form == "dual":
        o = o + branch(ops["b2"], st2)
    elif case.form == "res":
        o = o + ops["res"]
    return o


def bn_bwd_reference(case, ops, y, st1, st2):
    """float64 backward from the stored output y (None: no gate).  Returns gg (fp32: the gated gradient, one fp32 multiply under the leaky
    gate), dbeta, dgamma[, dgamma2] and dx[, dx2] in float64."""
    m = case.m
    gg = ops["g"] if y is None else act_gate(ops["g"], y.float(), case.act)
    g64 = gg.double()
    out = dict(gg=gg, dbeta=g64.sum(0))
    for key, b, st in (("", ops["b1"], st1), ("2", ops["b2"], st2)):
        if b is None:
            continue
        mean, rstd = st
        xc = b["x"].double() - mean[None, :]
        dgamma = (g64 * xc).sum(0) * rstd
        xhat = xc * rstd[None, :]
        gr = b["gamma"].double() * rstd
        out["dgamma" + key] = dgamma
        out["dx" + key] = gr[None, :] * (g64 - (out["dbeta"] / m)[None, :] - xhat * (dgamma / m)[None, :])
        out["terms" + key] = (gr, xhat, dgamma)
    return out


# dx = gr * ((gg - dbeta * inv_n) - xh * (dgamma * inv_n)) in bn_bwd_dx_kernel, gr = gamma * rs, xh = (x - mean) * rs, inv_n = 1.f / M.
# fp32 roundings, each a factor (1 + d), |d| <= 2^-24 (division and multiplication are correctly rounded; contraction only removes some):
#   d1: x - mean   d2: (.) * rs   d3: 1.f / M   d4: dbeta * inv_n   d5: dgamma * inv_n   d6: xh * (.)   d7: gg - (.)   d8: (.) - (.)
#   d9: gamma * rs   d10: gr * (.)  (for fp32 output this IS the output rounding)
# The term gg carries d7 d8 d9 d10 (4), dbeta / M carries d3 d4 d7 d8 d9 d10 (6), xh dgamma / M carries d1 d2 d3 d5 d6 d8 d9 d10 (8).
# With every term charged the largest count, |dx - exact| <= gamma_8 |gr| (|gg| + |dbeta| / M + |xh dgamma| / M), gamma_8 = 8u / (1 - 8u),
# u = 2^-24 (the standard bound for a product of eight such factors).  dbeta, dgamma and the statistics enter exactly: they are
# asserted bit for bit first.  bf16 output adds the one rounding to bf16: half a bf16 ulp of the reference.
DX_ROUNDINGS = 8


def dx_bound(ref, key, dtype, m):
    gr, xhat, dgamma = ref["terms" + key]
    u = 2.0 ** -24
    g8 = DX_ROUNDINGS * u / (1 - DX_ROUNDINGS * u)
    b = g8 * gr.abs()[None, :] * (ref["gg"].double().abs() + (ref["dbeta"].abs() / m)[None, :] + (xhat * dgamma[None, :]).abs() / m)
    if dtype == "bf16":
        b = b + 0.5 * ulp_bf16(ref["dx" + key])
    return b


def _r32(v64):
    return v64.float().double()


def dx_fp32_restatement(ref, key, b, st, m, order, fused=False):
    """dx in fp32 (values carried in float64, every operation rounded to fp32 by _r32).  order "kernel": the kernel's association;
    "distributed": gr gg - gr (dbeta inv_n) - (gr xh) (dgamma inv_n).  fused: a * b + c rounds once (the float64 product of two fp32 values
    is exact; its sum with c is rounded to fp32)."""
    mean, rstd = st
    gg = ref["gg"].double()
    dbeta, dgamma = _r32(ref["dbeta"]), _r32(ref["dgamma" + key])
    x = b["x"].double()
    rs = _r32(rstd)
    inv_n = float(np.float32(1.0) / np.float32(m))
    xh = _r32(_r32(x - _r32(mean)[None, :]) * rs[None, :])
    gr = _r32(b["gamma"].double() * rs)
    t2 = _r32(dgamma * inv_n)
    if order == "kernel":
        if fused:
            u = _r32(gg - (dbeta * inv_n)[None, :])
            w = _r32(u - xh * t2[None, :])
        else:
            u = _r32(gg - _r32(dbeta * inv_n)[None, :])
            w = _r32(u - _r32(xh * t2[None, :]))
        return _r32(gr[None, :] * w)
    t1 = _r32(gr * _r32(dbeta * inv_n))
    return _r32(_r32(_r32(gr[None, :] * gg) - t1[None, :]) - _r32(_r32(gr[None, :] * xh) * t2[None, :]))


def is_pow2(m):
    return m & (m - 1) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
WG_KT, WG_MAX_SPLITS = 64, 64                    # kWgKT, kWgMaxSplits
WG_RX, WG_RD, WG_RW = 8, 4, 64                   # |x|, |dy|, |accumulate base| at most


def pw_wgrad_plan(m, cin, cout):
    """pw_wgrad_plan of the library: (splits requested before the row rounding, splits launched, rows per split)."""
    tiles = (cin // 64) * (cout // 64)
    s = (1024 + tiles - 1) // tiles
    s = max(1, min(s, (m + 255) // 256, WG_MAX_SPLITS))
    rps = (m + s - 1) // s
    rps = (rps + WG_KT - 1) // WG_KT * WG_KT
    return s, (m + rps - 1) // rps, rps


# plan: (splits requested, splits launched, rows per split, rows of the last split) the case is in the table for
PwWgCase = collections.namedtuple("PwWgCase", "name n hc wc in_stride hin win cin cout accumulate seed plan")


def _pwwg(name, m, cin, cout, seed, plan, accumulate=False):
    return PwWgCase(name, 1, 1, m, 1, 1, m, cin, cout, accumulate, seed, plan)


def _pwwg_s2(n, hin, win, cin, cout, seed, accumulate=False):
    hc, wc = (hin - 1) // 2 + 1, (win - 1) // 2 + 1
    m = n * hc * wc
    return PwWgCase(f"gather{n}x{hin}x{win}-k{cin}-c{cout}", n, hc, wc, 2, hin, win, cin, cout, accumulate, seed, (1, 1, 64, m))


PW_WGRAD_CASES = [
    # fewer rows than one 64-row K stage, exactly one, one more
    _pwwg("m1-k64-c64", 1, 64, 64, 3001, (1, 1, 64, 1)),
    _pwwg("m63-k128-c192", 63, 128, 192, 3002, (1, 1, 64, 63)),
    _pwwg("m64-k192-c64", 64, 192, 64, 3003, (1, 1, 64, 64), accumulate=True),
    _pwwg("m65-k64-c64", 65, 64, 64, 3004, (1, 1, 128, 65)),
    _pwwg("m65-k128-c192", 65, 128, 192, 3005, (1, 1, 128, 65), accumulate=True),
    # two splits of 192 rows: the second holds one full stage and 44 rows
    _pwwg("m300-k64-c64", 300, 64, 64, 3006, (2, 2, 192, 108)),
    _pwwg("m300-k128-c192", 300, 128, 192, 3007, (2, 2, 192, 108)),
    _pwwg("m300-k192-c64", 300, 192, 64, 3008, (2, 2, 192, 108), accumulate=True),
    # the 64-split cap: 16454 rows ask for 65 splits, get 64 requested, and 320-row splits make that 52 launched with 134 rows last;
    # 20230 rows launch all 64, the last with one stage and 6 rows
    _pwwg("m16454-k64-c64", 16384 + 70, 64, 64, 3009, (64, 52, 320, 134)),
    _pwwg("m16454-k128-c192", 16384 + 70, 128, 192, 3010, (64, 52, 320, 134), accumulate=True),
    _pwwg("m20230-k192-c64", 20230, 192, 64, 3011, (64, 64, 320, 70)),
    # the stride-2 gather of the downsample conv; the skipped pixels hold NaN
    _pwwg_s2(2, 5, 7, 128, 192, 3012),
    _pwwg_s2(3, 6, 6, 64, 64, 3013, accumulate=True),
    _pwwg_s2(2, 7, 4, 192, 64, 3014),
]


def pw_wgrad_operands(c):
    """x (N, Cin, Hin, Win) with NaN at the pixels a stride-2 gather skips, dy (N, Cout, Hc, Wc), dw0 (Cout, Cin)."""
    x = ints((c.n, c.cin, c.hin, c.win), -WG_RX, WG_RX, c.seed)
    if c.in_stride == 2:
        keep = torch.zeros(c.hin, c.win, dtype=torch.bool)
        keep[::2, ::2] = True
        x = torch.where(keep[None, None], x, torch.full_like(x, float("nan")))
    return dict(x=x, dy=ints((c.n, c.cout, c.hc, c.wc), -WG_RD, WG_RD, c.seed + 500), dw0=ints((c.cout, c.cin), -WG_RW, WG_RW, c.seed + 700))


def pw_wgrad_bound(c):
    return c.n * c.hc * c.wc * WG_RX * WG_RD + WG_RW


def pw_wgrad_reference(c, ops, acc=torch.float32):
    xs = ops["x"][:, :, ::c.in_stride, ::c.in_stride]
    assert xs.shape[2:] == (c.hc, c.wc) and not bool(torch.isnan(xs).any())
    dw = torch.einsum("nohw,nihw->oi", ops["dy"].to(acc), xs.to(acc))
    return ops["dw0"].to(acc) + dw if c.accumulate else dw


def tiles_that_differ(got, want):
    """[(cout tile, cin tile, elements)] of the 64 x 64 tiles in which two (Cout, Cin) matrices differ."""
    bad = (got != want) | torch.isnan(got)
    out = []
    for co in range(0, bad.shape[0], 64):
        for ci in range(0, bad.shape[1], 64):
            k = int(bad[co:co + 64, ci:ci + 64].sum())
            if k:
                out.append((co // 64, ci // 64, k))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# stem weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
ST_P, ST_TAPS, ST_MAX_SPLITS = 32, 147, 512      # kStP, kStTaps, kStMaxSplits


def stem_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def stem_wgrad_plan(n, h, w):
    """stem_wgrad_plan of the library: (splits, output pixels per split)."""
    ho, wo = stem_out(h, w)
    p = n * ho * wo
    s = max(1, min((p + 255) // 256, ST_MAX_SPLITS))
    pps = (p + s - 1) // s
    pps = (pps + ST_P - 1) // ST_P * ST_P
    return (p + pps - 1) // pps, pps


StemWgCase = collections.namedtuple("StemWgCase", "name n h w accumulate seed plan")
STEM_WGRAD_CASES = [
    StemWgCase("1x1x1", 1, 1, 1, False, 4001, (1, 32)),
    StemWgCase("1x7x7", 1, 7, 7, True, 4002, (1, 32)),
    StemWgCase("2x9x6", 2, 9, 6, False, 4003, (1, 32)),
    StemWgCase("1x33x40", 1, 33, 40, True, 4004, (2, 192)),          # 340 pixels: 192 + 148 (four stages and 20 pixels)
    StemWgCase("3x61x47", 3, 61, 47, False, 4005, (9, 256)),         # 2232 pixels: eight full splits and 184
    StemWgCase("8x256x256", 8, 256, 256, True, 4006, (512, 256)),    # 131072 pixels: the 512-split cap
]
ST_RX, ST_RD, ST_RW = 8, 4, 64


def stem_wgrad_operands(c):
    ho, wo = stem_out(c.h, c.w)
    return dict(x=ints((c.n, 3, c.h, c.w), -ST_RX, ST_RX, c.seed), dy=ints((c.n, 64, ho, wo), -ST_RD, ST_RD, c.seed + 500),
                dw0=ints((64, 3, 7, 7), -ST_RW, ST_RW, c.seed + 700))


def stem_wgrad_bound(c):
    ho, wo = stem_out(c.h, c.w)
    return c.n * ho * wo * ST_RX * ST_RD + ST_RW


def stem_wgrad_reference(c, ops, acc=torch.float32):
    dw = torch.nn.grad.conv2d_weight(ops["x"].to(acc), (64, 3, 7, 7), ops["dy"].to(acc), stride=2, padding=3)
    return ops["dw0"].to(acc) + dw if c.accumulate else dw


# ---------------------------------------------------------------------------------------------------------------------------------
# maxpool3s2
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_GRID_CAP = 256 * 16                         # grid_cap: workgroups of 256 threads at most
PoolCase = collections.namedtuple("PoolCase", "name dtype n c h w halves nans seed")


def _pool_cases():
    out, seed = [], 5000
    for h, w in ((1, 1), (1, 6), (2, 2), (7, 5), (8, 8), (45, 70)):
        for dtype in ("bf16", "fp32"):
            for c in (64, VEC[dtype]):
                seed += 1
                out.append(PoolCase(f"{dtype}-c{c}-{h}x{w}", dtype, 2, c, h, w, False, False, seed))
    out.append(PoolCase("bf16-c64-7x5-halves", "bf16", 2, 64, 7, 5, True, False, 5101))
    out.append(PoolCase("fp32-c64-8x8-nan", "fp32", 2, 64, 8, 8, False, True, 5102))
    return out


POOL_CASES = _pool_cases()
# total vectors > 256 * 16 * 256, so the grid-stride loops run more than once: backward over the input pixels, forward over the output's
POOL_BWD_BIG = PoolCase("fp32-c64-192x192-gridstride", "fp32", 2, 64, 192, 192, False, False, 5201)
POOL_FWD_BIG = PoolCase("fp32-c64-364x364-gridstride", "fp32", 2, 64, 364, 364, False, False, 5202)


def pool_operands(c):
    """x: integers in [-2, 2] (most windows tie; zeros for the ReLU gate), optionally with +-1/2 on a fifth of the sites or a few NaN;
    dy: integers in [-4, 4]."""
    ho, wo = stem_out(c.h, c.w)
    gen = torch.Generator().manual_seed(c.seed)
    x = torch.randint(-2, 3, (c.n, c.c, c.h, c.w), generator=gen).float()
    if c.halves:
        x = x + torch.where(torch.rand(x.shape, generator=gen) < 0.2, 0.5, 0.0) * torch.where(torch.rand(x.shape, generator=gen) < 0.5, -1.0, 1.0)
    if c.nans:
        x = torch.where(torch.rand(x.shape, generator=gen) < 0.03, torch.full_like(x, float("nan")), x)
    return dict(x=x, dy=torch.randint(-4, 5, (c.n, c.c, ho, wo), generator=gen).float())


def pool_forward_restatement(x):
    """The kernel's rule, tap by tap in scan order over the in-bounds taps of each window: take the tap if it is the first, if it is
    larger, or if it is NaN.  So: the first maximum; with NaN in the window, NaN and the LAST NaN tap.  Returns (y (N, C, Ho, Wo) fp32,
    argmax (N, Ho, Wo, C) uint8, window-local kh * 3 + kw)."""
    n, c, h, w = x.shape
    ho, wo = stem_out(h, w)
    xp = F.pad(x, (1, 2, 1, 2), value=0.0)
    inb = F.pad(torch.ones(h, w, dtype=torch.bool), (1, 2, 1, 2), value=False)
    m = torch.full((n, c, ho, wo), float("-inf"))
    am = torch.zeros((n, c, ho, wo), dtype=torch.uint8)
    first = torch.ones((ho, wo), dtype=torch.bool)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, :, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2]
            valid = inb[kh:kh + 2 * ho:2, kw:kw + 2 * wo:2]
            take = valid[None, None] & (first[None, None] | (v > m) | torch.isnan(v))
            m = torch.where(take, v, m)
            am = torch.where(take, torch.full_like(am, kh * 3 + kw), am)
            first = first & ~valid
    assert not bool(first.any())                 # every window has its centre tap
    return m, am.permute(0, 2, 3, 1).contiguous()


def pool_backward_restatement(dy, argmax, h, w):
    """dx (N, C, H, W): each window's gradient goes to the tap its stored arg-max names."""
    n, c, ho, wo = dy.shape
    am = argmax.permute(0, 3, 1, 2).long()
    oh = torch.arange(ho)[None, None, :, None]
    ow = torch.arange(wo)[None, None, None, :]
    ih, iw = 2 * oh - 1 + am // 3, 2 * ow - 1 + am % 3
    assert bool(((ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)).all())
    nn_ = torch.arange(n)[:, None, None, None].expand_as(am)
    cc = torch.arange(c)[None, :, None, None].expand_as(am)
    dx = torch.zeros(n, c, h, w)
    dx.index_put_((nn_, cc, ih.expand_as(am), iw.expand_as(am)), dy, accumulate=True)
    return dx


def pool_autograd(x, dy):
    """(y, dx) of torch's F.max_pool2d(3, 2, 1) on the CPU in fp32."""
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    y.backward(dy)
    return y.detach(), xr.grad


def tie_share(x):
    """Share of windows whose maximum occurs at more than one in-bounds tap (where the tie rule decides the arg-max)."""
    n, c, h, w = x.shape
    ho, wo = stem_out(h, w)
    y = F.max_pool2d(x, 3, 2, 1)
    xp = F.pad(x, (1, 2, 1, 2), value=float("-inf"))
    cnt = torch.zeros_like(y)
    for kh in range(3):
        for kw in range(3):
            cnt += (xp[:, :, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] == y).float()
    return float((cnt > 1).double().mean())
