"""The spectral-norm oracles of tests/_sn_ref.py checked on the CPU: the closed forms are stock torch.nn.utils.spectral_norm, every exact
case satisfies its premise and is independent of the summation order, a correct fp32 evaluation passes every check, and the faults
these tests exist for (a dropped row or column, an unnormalised v, swapped u / v indices, a forgotten 1 / sigma^2) fail them."""
import numpy as np
import pytest

import _sn_ref as R

SMALL = [s for s in R.POWER_SHAPES if s[0] * s[1] <= 150000]
TOL_SHAPES = [(4, 1), (9, 3), (3, 27), (1, 512), (33, 257), (70, 600)]


def _gauss(rows, cols, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((rows, cols)) * 0.1).astype(np.float32)
    u = rng.standard_normal(rows)
    v = rng.standard_normal(cols)
    G = rng.standard_normal((rows, cols)).astype(np.float32)
    return W, (u / np.linalg.norm(u)).astype(np.float32), (v / np.linalg.norm(v)).astype(np.float32), G


@pytest.mark.parametrize("rows,cols", TOL_SHAPES)
def test_closed_forms_are_stock_spectral_norm(rows, cols):
    W, u, v, G = _gauss(rows, cols, 1)
    stock = R.StockSN(W, 1e-12)
    for train in (True, True, False):
        ref = stock.step(u, v, train, G)
        mine = R.forward64(W, u, v, train, 1e-12)
        for key in ("u", "v", "w_eff"):
            np.testing.assert_allclose(mine[key], ref[key], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(R.backward64(G, W, mine["u"], mine["v"], mine["sigma"]), ref["dw"], rtol=1e-11, atol=1e-14)
        u, v = ref["u"].astype(np.float32), ref["v"].astype(np.float32)


def test_zero_weight_semantics_are_stock():
    """sigma = 0, W / sigma all NaN, u and v zero: what the stock module gives, and what check_zero pins."""
    W = np.zeros((3, 7), dtype=np.float32)
    _, u, v, _ = _gauss(3, 7, 2)
    ref = R.StockSN(W, 1e-12).step(u, v, True)
    assert np.isnan(ref["w_eff"]).all() and not ref["u"].any() and not ref["v"].any()
    R.check_zero(3, 7, R.forward32(W, u, v, 1, 1e-12, np.random.default_rng(0)))


@pytest.mark.parametrize("rows,cols", R.POWER_SHAPES)
def test_power_case_premise_and_closed_form(rows, cols):
    c = R.power_case(rows, cols, 7)
    ref = R.forward64(c["W"], c["u"], c["v0"], 1, c["eps"])
    assert np.array_equal(ref["v"], c["v"]) and np.array_equal(ref["u_raw"], c["u_raw"]) and np.array_equal(ref["v_raw"], c["v_raw"])
    assert abs(ref["sigma"] - c["sigma"]) <= 1e-13 * c["sigma"]
    np.testing.assert_allclose(ref["u"], c["u_new"], rtol=1e-13, atol=0)
    assert np.abs(c["W"]).max() >= 1 and len(set(c["reserved"])) == 4
    assert all(np.count_nonzero(c["W"][:, j]) <= 1 for j in c["reserved"])
    # the reserved columns are spread over the range, not the last four
    assert c["reserved"][0] < cols / 4 and c["reserved"][-1] >= cols // 2


@pytest.mark.parametrize("rows,cols", SMALL)
def test_power_case_is_order_independent(rows, cols):
    c = R.power_case(rows, cols, 7)
    for seed in range(3):
        got = R.forward32(c["W"], c["u"], c["v0"], 1, c["eps"], np.random.default_rng(seed))
        R.check_power(c, got)


@pytest.mark.parametrize("rows,cols", R.POWER_SHAPES + R.NARROW_SHAPES)
def test_iter0_case(rows, cols):
    c = R.iter0_case(rows, cols, 3)
    assert R.forward64(c["W"], c["u"], c["v"], 0, c["eps"])["sigma"] == c["sigma"]
    if rows * cols <= 150000:
        for seed in range(3):
            R.check_iter0(c, R.forward32(c["W"], c["u"], c["v"], 0, c["eps"], np.random.default_rng(seed)))


CLAMPS = [((33, 257), -10, 24, False), ((70, 600), -10, 24, False), ((3, 27), 3, 10, True), ((33, 257), 3, 10, True), ((1, 5), -6, 24, True)]


@pytest.mark.parametrize("shape,k,s,u_clamped", CLAMPS)
def test_clamp_case(shape, k, s, u_clamped):
    c = R.clamp_case(*shape, 5, k, s)
    assert c["u_clamped"] == u_clamped
    ref = R.forward64(c["W"], c["u"], c["v0"], 1, c["eps"])
    assert np.array_equal(ref["v"], c["v"])
    np.testing.assert_allclose(ref["u"], c["u_new"], rtol=1e-13, atol=0)
    assert abs(ref["sigma"] - c["sigma"]) <= 1e-13 * c["sigma"]
    for seed in range(3):
        R.check_clamp(c, R.forward32(c["W"], c["u"], c["v0"], 1, c["eps"], np.random.default_rng(seed)))


@pytest.mark.parametrize("rows,cols", R.POWER_SHAPES + R.NARROW_SHAPES)
@pytest.mark.parametrize("a", [3, -2])
def test_bwd_case(rows, cols, a):
    c = R.bwd_case(rows, cols, 9, a)
    assert np.array_equal(R.backward64(c["G"], c["W"], c["u"], c["v"], float(c["sigma"][0])), c["dw"])
    if rows * cols <= 150000:
        for seed in range(3):
            R.check_bwd(c, R.backward32(c["G"], c["W"], c["u"], c["v"], c["sigma"], np.random.default_rng(seed)))


# ---------------------------------------------------------------------------------------------------------------------------------
# tolerance tier: a correct fp32 evaluation is inside the derived bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def _tolerance_run(rows, cols, forward, backward):
    """Three training steps and one eval step as tests/test_gpu_spectral_norm.py runs them; forward / backward: the implementation."""
    W, u, v, G = _gauss(rows, cols, 4)
    stock = R.StockSN(W, 1e-12)
    worst = 0.0
    for step, train in enumerate((True, True, True, False)):
        ref = stock.step(u, v, train, G)
        fb = R.forward_bounds(W, u, v, train)
        got = forward(W, u, v, train)
        got["dw"] = backward(G, W, got["u"], got["v"], got["sigma"])
        worst = max(worst, R.check_tolerance(f"{rows}x{cols} step {step}", ref, fb, got, R.backward_bounds(G, W, fb)))
        u, v = got["u"], got["v"]
    return worst


@pytest.mark.parametrize("rows,cols", TOL_SHAPES)
def test_fp32_evaluation_is_inside_the_tolerance_bounds(rows, cols):
    rng = np.random.default_rng(0)
    _tolerance_run(rows, cols, lambda W, u, v, t: R.forward32(W, u, v, t, 1e-12, rng), lambda *a: R.backward32(*a, rng))


# ---------------------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
def _finish32(b, eps):
    tot = np.float32(np.sum(b.astype(np.float64) ** 2))
    inv = np.float32(1) / max(np.sqrt(tot), np.float32(eps))
    return b * inv, np.array([tot * inv, np.float32(1) / (tot * inv)], dtype=np.float32)


def _faulty_forward(fault):
    def run(W, u, v, power_iter, eps=1e-12):
        rng = np.random.default_rng(0)
        rows, cols = W.shape
        W2 = W.copy()
        if fault == "row":                           # the last row of a 32-row group never read
            W2[min(31, rows - 1)] = 0
        if fault == "col":                           # column 256, the first of the second column block, never read
            W2[:, 256] = 0
        out = R.forward32(W2, u, v, power_iter, eps, rng)
        if fault == "raw_v" and power_iter:          # W v taken from v before its normalisation
            b = (W.astype(np.float64) @ out["v_raw"].astype(np.float64)).astype(np.float32)
            out["u_raw"] = b
            out["u"], out["sigma"] = _finish32(b, eps)
        out["w_eff"] = W * out["sigma"][1]
        return out
    return run


def _faulty_backward(fault):
    def run(G, W, u, v, sigma):
        rows, cols = W.shape
        sigma = np.asarray(sigma, dtype=np.float32)
        if fault == "swap":                          # u indexed by the column, v by the row
            i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
            dot = np.float32(np.sum(G.astype(np.float64) * W))
            return G * sigma[1] - dot * sigma[1] * sigma[1] * u[j % rows] * v[i % cols]
        if fault == "sigma2":                        # <G, W> not divided by sigma^2
            dot = np.float32(np.sum(G.astype(np.float64) * W))
            return G * sigma[1] - dot * u[:, None] * v[None, :]
        return R.backward32(G, W, u, v, sigma, np.random.default_rng(0))
    return run


@pytest.mark.parametrize("fault,shapes", [("row", [(33, 257), (70, 600), (260, 300)]), ("col", [(33, 257), (70, 600), (129, 1153)]),
                                          ("raw_v", [(3, 27), (33, 257), (70, 600)])])
def test_planted_forward_faults_fail_every_check(fault, shapes):
    for rows, cols in shapes:
        c = R.power_case(rows, cols, 7)
        got = _faulty_forward(fault)(c["W"], c["u"], c["v0"], 1)
        # each pinned quantity on its own: the fault must move all of them out of their equality / bound
        keys = {"row": ("v", "u", "sigma"), "col": ("v", "u", "sigma"), "raw_v": ("sigma", "w_eff")}[fault]
        for key in keys:
            ok = dict(R.forward32(c["W"], c["u"], c["v0"], 1, c["eps"], np.random.default_rng(1)))
            R.check_power(c, ok)
            ok[key] = got[key]
            with pytest.raises(AssertionError):
                R.check_power(c, ok)
    for rows, cols in [s for s in shapes if s in TOL_SHAPES]:
        with pytest.raises(AssertionError):
            _tolerance_run(rows, cols, _faulty_forward(fault), _faulty_backward(None))
        # and at the FIRST step already, on the forward's own outputs
        W, u, v, G = _gauss(rows, cols, 4)
        ref, fb = R.StockSN(W, 1e-12).step(u, v, True), R.forward_bounds(W, u, v, True)
        with pytest.raises(AssertionError):
            R.check_tolerance("planted", ref, fb, _faulty_forward(fault)(W, u, v, True))


@pytest.mark.parametrize("fault", ["swap", "sigma2"])
def test_planted_backward_faults_fail_every_check(fault):
    for rows, cols in [(3, 27), (33, 257), (70, 600), (257, 40)]:
        for a in (3, -2):
            c = R.bwd_case(rows, cols, 9, a)
            with pytest.raises(AssertionError):
                R.check_bwd(c, _faulty_backward(fault)(c["G"], c["W"], c["u"], c["v"], c["sigma"]).astype(np.float32))
    for rows, cols in [(3, 27), (33, 257), (70, 600)]:
        rng = np.random.default_rng(0)
        with pytest.raises(AssertionError):
            _tolerance_run(rows, cols, lambda W, u, v, t: R.forward32(W, u, v, t, 1e-12, rng), _faulty_backward(fault))


def test_four_squares_and_reserved_columns():
    for d in list(range(0, 200)) + [4 ** 8 - 37211, 4 ** 10 - 1, 4 ** 11 - 12345]:
        assert sum(x * x for x in R.four_squares(d)) == d
    for cols in (5, 6, 27, 255, 256, 257, 1153):
        assert len(set(R.reserved_columns(cols))) == 4
