"""The premises of tests/test_gpu_train_exact.py, proven on the CPU for every case of tests/_train_ref.py: the data is balanced (mean and
variance are the designed ones), every sum stays below 2^24 on its grid, the kernels' operation order in fp32 equals float64, the split
counts each case is in the table for are the ones the restated launch arithmetic gives, and the references contain what makes a wrong
kernel visible (values bf16 cannot hold, exact zeros before the ReLU, tied windows)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _train_ref as R

BN_IDS = [c.name for c in R.BN_CASES]


@functools.lru_cache(maxsize=2)
def _bn_by_name(name):
    case = R.BN_BY_NAME[name]
    ops = R.bn_operands(case)
    st1 = R.bn_stats_reference(case, ops["b1"])
    st2 = R.bn_stats_reference(case, ops["b2"]) if ops["b2"] is not None else None
    return ops, st1, st2


def _bn(case):
    return _bn_by_name(case.name)


@pytest.mark.parametrize("case", R.BN_CASES, ids=BN_IDS)
def test_bn_data_is_balanced_and_the_sums_are_exact(case):
    ops, st1, st2 = _bn(case)
    for b, st in ((ops["b1"], st1), (ops["b2"], st2)):
        if b is None:
            continue
        mean, var, rstd = st
        x = b["x"]
        assert torch.equal(x.bfloat16().float(), x)                              # bf16 holds every input
        assert torch.equal(mean, b["m"].double())
        assert torch.equal(var, (b["a"].double() ** 2) if case.m > 1 else torch.zeros(case.c, dtype=torch.float64))
        want_rstd = 1.0 / b["a"].double() if case.eps == 0 else torch.full((case.c,), 1.0 / (float(var[0]) + case.eps) ** 0.5, dtype=torch.float64)
        assert torch.equal(rstd, want_rstd)
        assert bool((torch.log2(rstd) == torch.log2(rstd).round()).all())        # a power of two
        s1, s2 = R.stats_bounds(x)
        assert s1 < R.TWO24 and s2 < R.TWO24
        # the kernel's arithmetic in fp32: shifted sums in permuted chunks of 37 rows, then s / n and the mean, against float64
        k = x[0]
        d = x - k[None, :]
        perm = torch.randperm(case.m, generator=torch.Generator().manual_seed(case.seed))
        p1, p2 = torch.zeros(case.c), torch.zeros(case.c)
        for chunk in perm.split(max(1, case.m // 37)):
            p1 = p1 + d[chunk].sum(0)
            p2 = p2 + (d[chunk] * d[chunk]).sum(0)
        assert torch.equal(p1.double(), d.double().sum(0)) and torch.equal(p2.double(), (d.double() ** 2).sum(0))
        n = float(case.m)
        dm = p1.double() / n
        assert torch.equal(k.double() + dm, mean)
        assert torch.equal((p2.double() / n - dm * dm).clamp_min(0.0), var)
        R.stats_tensor(mean, rstd)
    rm, rv = R.running_reference(case, ops, st1[0], st1[1])
    assert torch.equal(rm.double(), case.momentum * st1[0] + (1 - case.momentum) * ops["running_mean0"].double())
    # the fp32 restatement of running_var, unfused and fused, is inside the stated ulps
    unb = (st1[1] * n / (n - 1.0) if case.m > 1 else st1[1]).float()
    mom = torch.tensor(case.momentum)
    unfused = mom * unb + (1 - mom) * ops["running_var0"]
    fused = (mom.double() * unb.double() + ((1 - mom) * ops["running_var0"]).double()).float()
    for got in (unfused, fused):
        assert bool(((got.double() - rv).abs() <= R.RUNNING_VAR_ULPS * R.ulp32(rv)).all())


def test_bn_split_arithmetic():
    """Every case reaches the split geometry it is in the table for; the empty last split and the clamp are really there."""
    for case in R.BN_CASES:
        for dtype in case.dtypes:
            splits, rps, last = R.bn_plan(case.m, case.c, dtype)
            assert (splits, last) == case.plan[dtype], (case.name, dtype, splits, rps, last)
    assert R.bn_plan(32770, 64, "fp32") == (256, 129, -125) and 255 * 129 > 32770 > 254 * 129
    assert R.bn_plan(512, 64, "bf16")[0] == 2 and R.bn_plan(4096, 64, "bf16")[:2] == (16, 256) and R.bn_plan(4096, 192, "bf16")[:2] == (16, 256)
    assert R.bn_plan(4100, 64, "bf16")[1:] == (257, 245)
    # the clamp: 2^16 rows ask for exactly 256 bf16 splits (cap = M / 256), 2^17 for 512
    assert 65536 // (8 * R.BN_RP["bf16"]) == 256 and 131072 // (8 * R.BN_RP["bf16"]) == 512 and R.bn_splits(131072, 64, "bf16") == 256
    big = R.BN_CASES[-1]
    assert big.m * (big.c // R.VEC["fp32"]) > R.EW_GRID_CAP * 256
    assert {1, 2, 30, 512, 4096, 4100, 32770, 65536, 131072} == {c.m for c in R.BN_CASES}


@pytest.mark.parametrize("case", R.BN_CASES, ids=BN_IDS)
def test_bn_apply_oracle_is_exact_and_shows_a_wrong_kernel(case):
    ops, st1, st2 = _bn(case)
    s1 = (st1[0], st1[2])
    s2 = (st2[0], st2[2]) if st2 is not None else None
    lin, out = R.bn_apply_reference(case, ops, s1, s2)
    assert torch.equal(R.bn_apply_fp32_restatement(case, ops, s1, s2), lin)      # the kernel's fp32 order loses nothing
    assert float(lin.abs().max()) <= 512
    if case.act != R.NONE:
        assert int((lin == 0).sum()) > 0                                         # exact zeros before the activation
    if case.form == "res":
        # the single rounding to bf16 is exercised: 128..255 plus a half needs nine bits.  Without a residual the designed output is at
        # most 16 on a grid of 1/2, which bf16 holds: the apply's rounding shows in the residual cases only (the backward's in every dx, test_bn_backward_oracle)
        assert R.unrepresentable(out) >= 0.01
    if case.act == R.LEAKY:
        assert int((lin < 0).sum()) > 0


def test_leaky_slope_premise():
    """0.2f v == v / 5 in fp32 for every multiple of 5 up to 2^10: on such values the kernel's single multiply equals the real-number
    LeakyReLU.  Elsewhere 0.2f v is not v / 5 (0.2f is not 1/5), which is why the oracle performs the same fp32 multiply and the exact
    LeakyReLU apply cases store fp32."""
    v = torch.arange(-1024, 1025, dtype=torch.float32)
    v5 = v[(v % 5) == 0]
    assert torch.equal((v5 * R.SLOPE).double(), v5.double() / 5)
    assert R.SLOPE.dtype == torch.float32 and float(R.SLOPE) == float(np.float32(0.2))
    other = v[(v % 5) != 0]
    assert int(((other * R.SLOPE).double() != other.double() * 0.2).sum()) > 0
    for c in R.BN_CASES:
        assert c.act != R.LEAKY or c.form == "res"


@pytest.mark.parametrize("case", R.BN_CASES, ids=BN_IDS)
def test_bn_backward_oracle(case):
    """dbeta / dgamma exact for any M; dx exact in fp32 (two association orders) where M is a power of two; elsewhere the fp32
    restatements, unfused and fused, inside the derived bound on EVERY element."""
    ops, st1, st2 = _bn(case)
    s1 = (st1[0], st1[2])
    s2 = (st2[0], st2[2]) if st2 is not None else None
    _, out = R.bn_apply_reference(case, ops, s1, s2)
    seen = None
    for dtype in case.dtypes:
        y = None if case.act == R.NONE else out.to(R.TORCH_DTYPE[dtype])
        if seen is not None and (y is None or torch.equal(R.act_gate(ops["g"], y.float(), case.act), seen)) and (R.is_pow2(case.m) or dtype == "fp32"):
            continue                                                             # the same gated gradient: the same oracle
        ref = R.bn_bwd_reference(case, ops, y, s1, s2)
        seen = ref["gg"]
        if y is not None:
            assert int((y == 0).sum()) > 0                                       # the gate is decided AT zero somewhere
        if case.act == R.LEAKY:
            continue                                                             # 0.2f g is not dyadic: only gres is compared
        assert float(ref["dbeta"].abs().max()) < R.TWO24 and float((ops["g"].abs().sum(0)).max()) < R.TWO24
        for key, b, st in (("", ops["b1"], s1), ("2", ops["b2"], s2)):
            if b is None:
                continue
            xc = b["x"].double() - st[0][None, :]
            assert float(((ref["gg"].double() * xc).abs() * 2).sum(0).max()) < R.TWO24       # sum gg (x - mean) on its grid of 1/2
            assert torch.equal(ref["dgamma" + key].float().double(), ref["dgamma" + key])
            dx = ref["dx" + key]
            if R.is_pow2(case.m):
                for order in ("kernel", "distributed"):
                    assert torch.equal(R.dx_fp32_restatement(ref, key, b, st, case.m, order), dx), (case.name, order)
                assert torch.equal(R.dx_fp32_restatement(ref, key, b, st, case.m, "kernel", fused=True), dx)
                if dtype == "bf16" and case.m >= 512:
                    assert R.unrepresentable(dx.float()) >= 0.25                 # the final rounding has work to do
            else:
                bound = R.dx_bound(ref, key, "fp32", case.m)
                for fused in (False, True):
                    got = R.dx_fp32_restatement(ref, key, b, st, case.m, "kernel", fused=fused)
                    assert bool(((got - dx).abs() <= bound).all()), (case.name, fused)
                # and the rounding to bf16 of such a value stays inside the bf16 bound
                got16 = R.dx_fp32_restatement(ref, key, b, st, case.m, "kernel").float().bfloat16().double()
                assert bool(((got16 - dx).abs() <= R.dx_bound(ref, key, "bf16", case.m)).all())


def test_ragged_and_power_of_two_rows_are_both_in_the_table():
    assert {c.m for c in R.BN_CASES if not R.is_pow2(c.m)} == {30, 4100, 32770}
    assert R.DX_ROUNDINGS == 8


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.PW_WGRAD_CASES, ids=lambda c: c.name)
def test_pointwise_wgrad_oracle(c):
    m = c.n * c.hc * c.wc
    req, splits, rps = R.pw_wgrad_plan(m, c.cin, c.cout)
    assert (req, splits, rps, m - (splits - 1) * rps) == c.plan
    assert R.pw_wgrad_bound(c) < R.TWO24
    ops = R.pw_wgrad_operands(c)
    assert torch.equal(R.pw_wgrad_reference(c, ops).double(), R.pw_wgrad_reference(c, ops, torch.float64))
    if c.in_stride == 2:
        skipped = torch.isnan(ops["x"])
        assert int(skipped.sum()) > 0 and not bool(skipped[:, :, ::2, ::2].any())


def test_pointwise_wgrad_table_covers_the_issue():
    rows = {c.n * c.hc * c.wc for c in R.PW_WGRAD_CASES if c.in_stride == 1}
    assert {1, 63, 64, 65, 300, 16384 + 70} <= rows
    assert {(c.cin, c.cout) for c in R.PW_WGRAD_CASES} == {(64, 64), (128, 192), (192, 64)}
    assert {(c.hin, c.win) for c in R.PW_WGRAD_CASES if c.in_stride == 2} == {(5, 7), (6, 6), (7, 4)}
    assert any(c.plan[0] == R.WG_MAX_SPLITS for c in R.PW_WGRAD_CASES) and any(c.plan[1] == R.WG_MAX_SPLITS for c in R.PW_WGRAD_CASES)
    assert R.pw_wgrad_plan(300, 64, 64) == (2, 2, 192) and 300 - 192 == 64 + 44


@pytest.mark.parametrize("c", R.STEM_WGRAD_CASES, ids=lambda c: c.name)
def test_stem_wgrad_oracle(c):
    assert R.stem_wgrad_plan(c.n, c.h, c.w) == c.plan
    assert R.stem_wgrad_bound(c) < R.TWO24
    ops = R.stem_wgrad_operands(c)
    ref = R.stem_wgrad_reference(c, ops)
    assert torch.equal(ref.double(), R.stem_wgrad_reference(c, ops, torch.float64))
    if c.n * c.h * c.w <= 4096:      # the definition, independently of torch's gradient routine
        xp = F.pad(ops["x"].double(), (3, 3, 3, 3))
        ho, wo = R.stem_out(c.h, c.w)
        dw = torch.zeros(64, 3, 7, 7, dtype=torch.float64)
        for kh in range(7):
            for kw in range(7):
                dw[:, :, kh, kw] = torch.einsum("nohw,nihw->oi", ops["dy"].double(), xp[:, :, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2])
        assert torch.equal(ref.double(), dw + (ops["dw0"].double() if c.accumulate else 0))


def test_stem_wgrad_table_covers_the_issue():
    assert [(c.n, c.h, c.w) for c in R.STEM_WGRAD_CASES] == [(1, 1, 1), (1, 7, 7), (2, 9, 6), (1, 33, 40), (3, 61, 47), (8, 256, 256)]
    assert R.STEM_WGRAD_CASES[-1].plan[0] == R.ST_MAX_SPLITS


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.POOL_CASES + [R.POOL_BWD_BIG], ids=lambda c: c.name)
def test_maxpool_restatement_agrees_with_torch(c):
    """The restated rule gives torch's maximum, and torch's autograd sends every window's gradient -- ties included -- to the tap the
    restated arg-max names."""
    ops = R.pool_operands(c)
    x, dy = ops["x"], ops["dy"]
    assert torch.equal(x.to(R.TORCH_DTYPE[c.dtype]).float().nan_to_num(nan=7.0), x.nan_to_num(nan=7.0))
    y, am = R.pool_forward_restatement(x)
    ty, tdx = R.pool_autograd(x, dy)
    assert torch.equal(torch.isnan(y), torch.isnan(ty)) and torch.equal(y.nan_to_num(nan=7.0), ty.nan_to_num(nan=7.0))
    assert int(am.max()) <= 8
    if c.nans:
        assert int(torch.isnan(ty).sum()) > 0 and int((~torch.isnan(ty)).sum()) > 0
        return                                                                   # the index under NaN is the kernel's rule alone
    assert torch.equal(R.pool_backward_restatement(dy, am, c.h, c.w), tdx)
    if c.h * c.w >= 4:               # two taps of five values tie one time in five, nine taps far more often
        assert R.tie_share(x) > 0.15
    if c.h * c.w >= 45 * 70:
        assert R.tie_share(x) > 0.5
    if c.h * c.w * c.c >= 256:
        assert int((x == 0).sum()) > 0


def test_maxpool_table_covers_the_issue():
    assert {(c.h, c.w) for c in R.POOL_CASES} == {(1, 1), (1, 6), (2, 2), (7, 5), (8, 8), (45, 70)}
    assert {(c.dtype, c.c) for c in R.POOL_CASES} == {("bf16", 64), ("bf16", 8), ("fp32", 64), ("fp32", 4)}
    b, f = R.POOL_BWD_BIG, R.POOL_FWD_BIG
    assert b.n * b.h * b.w * (b.c // R.VEC[b.dtype]) > R.POOL_GRID_CAP * 256
    ho, wo = R.stem_out(f.h, f.w)
    assert f.n * ho * wo * (f.c // R.VEC[f.dtype]) > R.POOL_GRID_CAP * 256
