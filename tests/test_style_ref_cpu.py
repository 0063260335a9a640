"""The AdaIN style oracles of tests/_style_ref.py checked on the CPU: the closed forms are float64 autograd of the stock formulation,
every exact case satisfies its premise and is independent of the summation order, a correct fp32 evaluation passes every check, and a
dropped sample lane (n % 8 == 7) or a wrong row index k fails them."""
import numpy as np
import pytest

import _style_ref as R

# (N, C, nc): every N of {1, 7, 8, 9, 19}, C of {1, 3, 8, 40, 65}, nc of {1, 5, 31, 32}; N = 19 with C = 65 and nc = 32
SHAPES = [(1, 1, 1), (7, 3, 5), (8, 8, 31), (9, 40, 5), (19, 65, 32), (8, 3, 32), (9, 65, 1)]


def _gauss(N, C, nc, seed, bias=True):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)           # noqa: E731
    return dict(y=f(N, nc), w=f(4 * C, nc) * np.float32(0.3), b=f(4 * C) if bias else None, d_std=f(N, C), d_mean=f(N, C))


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_closed_forms_are_autograd(N, C, nc, bias):
    d = _gauss(N, C, nc, 1, bias)
    ref = R.autograd64(d["y"], d["w"], d["b"], 1e-5, d["d_std"], d["d_mean"])
    f = R.forward64(d["y"], d["w"], d["b"], 1e-5)
    np.testing.assert_allclose(f["y_std"], ref["y_std"], rtol=1e-12)
    np.testing.assert_allclose(f["y_mean"], ref["y_mean"], rtol=1e-12, atol=1e-15)
    b = R.backward64(d["d_std"], d["d_mean"], d["y"], f["y4"], f["y_std"], f["y_mean"])
    np.testing.assert_allclose(b["dw"], ref["dw"], rtol=1e-10, atol=1e-12)
    if bias:
        np.testing.assert_allclose(b["db"], ref["db"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_forward_case_is_order_independent(N, C, nc, bias):
    c = R.fwd_case(N, C, nc, 3, bias)
    assert 0 in c["flat"]
    for seed in range(3):
        R.check_fwd(c, R.forward32(c["y"], c["w"], c["b"], c["eps"], np.random.default_rng(seed)))


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("tier", ["a", "b"])
def test_backward_case_is_order_independent(N, C, nc, tier):
    c = R.bwd_case(N, C, nc, 5, tier)
    if tier == "b":
        assert not np.array_equal(c["dw"][0::4], c["dw"][1::4]) or C * N == 1, "tier b must tell the four rows of a channel apart"
    for seed in range(3):
        got = R.backward32(c["d_std"], c["d_mean"], c["y"], c["y4"], c["y_std"], c["y_mean"], np.random.default_rng(seed))
        R.check_bwd(c, got["dw"], got["db"], 0)
        R.check_bwd(c, got["dw"] + c["dw0"], got["db"] + c["db0"], 1)


def _tolerance(N, C, nc, bias, lanes=range(8), kmap=(0, 1, 2, 3)):
    """A correct fp32 evaluation (or one that only walks the sample lanes `lanes` / reads y4[..., kmap[k]]) against the bounds."""
    d = _gauss(N, C, nc, 2, bias)
    rng = np.random.default_rng(0)
    ref = R.autograd64(d["y"], d["w"], d["b"], 1e-5, d["d_std"], d["d_mean"])
    bounds = R.tolerance_bounds(d["y"], d["w"], d["b"], 1e-5, d["d_std"], d["d_mean"])
    f = R.forward32(d["y"], d["w"], d["b"], 1e-5, rng)
    keep = np.array([n for n in range(N) if n % 8 in lanes])
    b = R.backward32(d["d_std"][keep], d["d_mean"][keep], d["y"][keep], f["y4"][keep][..., list(kmap)], f["y_std"][keep], f["y_mean"][keep], rng)
    got = dict(y_std=f["y_std"], y_mean=f["y_mean"], dw=b["dw"], db=b["db"] if bias else None)
    return R.check_tolerance(f"N{N} C{C} nc{nc}", ref, bounds, got)


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_fp32_evaluation_is_inside_the_tolerance_bounds(N, C, nc, bias):
    assert _tolerance(N, C, nc, bias) < 1


@pytest.mark.parametrize("N,C,nc", [s for s in SHAPES if s[0] >= 8])
def test_planted_lane_fault_fails_every_check(N, C, nc):
    """The sample lane n % 8 == 7 dropped: outside the exact tiers and outside the tolerance bounds."""
    lanes = range(7)
    keep = np.array([n for n in range(N) if n % 8 != 7])
    for tier in ("a", "b"):
        c = R.bwd_case(N, C, nc, 5, tier)
        got = R.backward32(c["d_std"][keep], c["d_mean"][keep], c["y"][keep], c["y4"][keep], c["y_std"][keep], c["y_mean"][keep],
                           np.random.default_rng(0))
        with pytest.raises(AssertionError):
            R.check_bwd(c, got["dw"], None, 0)
        with pytest.raises(AssertionError):
            R.check_bwd(c, c["dw"], got["db"], 0)
    with pytest.raises(AssertionError):
        _tolerance(N, C, nc, True, lanes=lanes)


@pytest.mark.parametrize("N,C,nc", [s for s in SHAPES if s[0] > 1])
def test_planted_row_index_fault_fails(N, C, nc):
    """Row 4c + k reading y4[..., k ^ 1]: tier (b) and the tolerance tier see it (tier (a) cannot: d_std = 0 there)."""
    c = R.bwd_case(N, C, nc, 5, "b")
    got = R.backward32(c["d_std"], c["d_mean"], c["y"], c["y4"][..., [1, 0, 3, 2]], c["y_std"], c["y_mean"], np.random.default_rng(0))
    with pytest.raises(AssertionError):
        R.check_bwd(c, got["dw"], got["db"], 0)
    with pytest.raises(AssertionError):
        _tolerance(N, C, nc, True, kmap=(1, 0, 3, 2))


def test_forward_faults_fail():
    """A dropped last input feature (j = nc - 1) or a missing bias moves y4 / y_mean off the exact oracle and y_std beyond 4 ulp."""
    c = R.fwd_case(9, 40, 5, 3, True)
    rng = np.random.default_rng(0)
    w2 = c["w"].copy()
    w2[:, -1] = 0
    for got in (R.forward32(c["y"], w2, c["b"], c["eps"], rng), R.forward32(c["y"], c["w"], None, c["eps"], rng)):
        with pytest.raises(AssertionError):
            R.check_fwd(c, dict(y_mean=got["y_mean"], y_std=c["y_std"].astype(np.float32)))
        with pytest.raises(AssertionError):
            R.check_fwd(c, dict(y_mean=c["y_mean"], y_std=c["y_std"].astype(np.float32), y4=got["y4"]))
    got = R.forward32(c["y"], w2, c["b"], c["eps"], rng)
    with pytest.raises(AssertionError):
        R.check_fwd(c, dict(y_mean=c["y_mean"], y_std=got["y_std"]))
