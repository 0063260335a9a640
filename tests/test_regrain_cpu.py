"""The regraining pass and the linear colour maps without a GPU: the numpy restatement (tests/_regrain_ref.py) against hand-written values and
against its own properties, the host-only level rule of the library, and every argument check of the new keywords of wu.colour."""
import numpy as np
import pytest
import torch

import _colour_cases as CC
import _regrain_cases as CASES
import _regrain_ref as G


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


@pytest.mark.parametrize("args,want", CASES.LEVEL_CASES)
def test_level_sizes(args, want):
    from wu import _lib
    assert G.level_sizes(*args) == want
    assert _lib.load().wu_colour_regrain_levels(*args) == len(want)          # the host-only entry point applies the same rule


def test_level_rule_and_workspace_refuse_bad_arguments():
    from wu import _lib
    lib = _lib.load()
    for h, w, k, m in ((0, 4, 1, 0), (4, 0, 1, 0), (4, 4, 0, 0), (4, 4, 7, 0), (4, 4, 1, -1)):
        assert lib.wu_colour_regrain_levels(h, w, k, m) == 0
    big = (1 << 21) + 1
    for nimg, h, w, levels in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 1, big, 1), (1, 4, 4, 0), (1, 4, 4, 7)):
        assert lib.wu_colour_regrain_workspace_bytes(nimg, h, w, levels) == 0
    assert lib.wu_colour_regrain_workspace_bytes(2, 9, 7, 3) == 2 * 8 * (3 * 63 + 8 * 63 + 17 * 20 + 17 * 6)
    for nsets, n in ((0, 4), (65536, 4), (1, 0), (1, big)):
        assert lib.wu_colour_moments_workspace_bytes(nsets, n) == 0
    assert lib.wu_colour_moments_workspace_bytes(3, 4097) == 3 * 2 * 6 * 8


def test_down_and_up_on_hand_written_arrays():
    a = np.array([[1.0, 2.0], [3.0, 5.0], [7.0, 11.0]])                       # 3 x 2 -> 2 x 1: rows (1+3)/2, (2+5)/2 and the last row alone
    assert np.array_equal(G.down(a), np.array([[(2.0 + 3.5) * 0.5], [(7.0 + 11.0) * 0.5]]))
    b = np.array([[1.0], [2.0], [4.0], [8.0], [16.0]])                        # 5 x 1 -> 3 x 1
    assert np.array_equal(G.down(b), np.array([[1.5], [6.0], [16.0]]))
    c = np.array([[0.0], [8.0], [4.0]])                                       # 3 x 1 -> 5 x 1: far neighbours -1 (clamped), 1, 0, 2, 1
    assert np.array_equal(G.up(c, 5, 1), np.array([[0.0], [2.0], [6.0], [7.0], [5.0]]))
    d = np.array([[0.0], [8.0]])                                              # 2 x 1 -> 3 x 2: both columns read the one coarse column
    assert np.array_equal(G.up(d, 3, 2), np.array([[0.0, 0.0], [2.0, 2.0], [6.0, 6.0]]))
    e = np.array([[0.0, 16.0]])                                               # 1 x 2 -> 1 x 3
    assert np.array_equal(G.up(e, 1, 3), np.array([[0.0, 4.0, 12.0]]))
    assert np.array_equal(G.sh(a, -1, 1), np.array([[2.0, 2.0], [2.0, 2.0], [5.0, 5.0]]))


def test_identity_and_flat_inputs():
    # at most 116 iterations, each a few ulp of values near 1: 1e-12 is three orders above that; the restatement leaves 1.6e-15
    i0, _, _ = CASES.grain_fixture()
    assert np.abs(G.regrain(i0, i0) - i0).max() < 1e-12
    assert np.abs(G.regrain(i0, i0, replace=True) - i0).max() > 1e-3           # the published recursion does not: DESIGN.md section 6s.1
    flat0 = np.full((3, 45, 50), 0.3)
    flat_t = np.stack([np.full((45, 50), v) for v in (0.9, -0.2, 0.5)])
    assert np.abs(G.regrain(flat0, flat_t) - flat_t).max() < 1e-12


def test_transposition_and_channel_order():
    """A transposed pair gives the transposed result only up to rounding: down and up go rows first, and den, b and a add the neighbours in
    the order up, down, left, right, which a transposition turns into left, right, up, down.  Exchanging channels 0 and 1 is exact: the
    channels meet only in (q_0 + q_1) + q_2, and that sum commutes."""
    i0, _, it = CASES.grain_fixture(seed=8, h=50, w=66)
    want = G.regrain(i0, it)
    got = G.regrain(i0.transpose(0, 2, 1).copy(), it.transpose(0, 2, 1).copy()).transpose(0, 2, 1)
    assert np.abs(got - want).max() < 1e-12 and not np.array_equal(got, want)
    swap = [1, 0, 2]
    assert np.array_equal(G.regrain(i0[swap], it[swap])[swap], want)


def test_grain_fixture():
    i0, clean, it = CASES.grain_fixture()
    ir = G.regrain(i0, it)
    before, after = rms(it - clean), rms(ir - clean)
    print(f"grain fixture: rms {before:.5f} -> {after:.5f} ({before / after:.2f} x)")          # 0.03122 -> 0.01071 (2.91 x)
    assert after < before / 2


def test_fixed_sum_order_depends_on_the_length_alone():
    rng = np.random.RandomState(3)
    for n in (1, 2, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5):
        v = rng.uniform(-1, 1, n)
        assert abs(G.fixed_sum(v) - float(np.sum(v.astype(np.longdouble)))) <= 4 * n * 2.0 ** -53
        assert np.array_equal(G.fixed_sum(np.stack([v, v[::-1]])), [G.fixed_sum(v), G.fixed_sum(v[::-1].copy())])      # sets do not mix
    assert G.fixed_sum(np.array([1.0, 2.0 ** -53, 2.0 ** -53])) == 1.0         # lanes 0, 1, 2 fold as (1 + 2^-53) + 2^-53: an order, not a sum


def test_jacobi_against_eigvalsh():
    worst = 0.0
    for seed in range(200):
        rng = np.random.RandomState(seed)
        x = rng.randn(3, 3) * rng.uniform(0.01, 1, (3, 1))
        cov = x @ x.T
        lam, v = G.jacobi(cov)
        ref = np.linalg.eigvalsh(cov)
        worst = max(worst, float(np.abs(np.sort(lam) - ref).max() / ref.max()))
        assert np.abs(v @ v.T - np.eye(3)).max() < 1e-14
        assert np.abs((v * lam) @ v.T - cov).max() <= 1e-14 * ref.max()
    assert worst < 1e-14                                                       # measured 9.7e-16
    lam, v = G.jacobi(np.diag([3.0, 1.0, 2.0]))                                # nothing to rotate: every rotation is skipped
    assert np.array_equal(lam, [3.0, 1.0, 2.0]) and np.array_equal(v, np.eye(3))
    low = np.array([[2.0, 0.5, 0.0], [99.0, 1.0, 0.25], [99.0, 99.0, 3.0]])    # only the upper triangle is read
    assert np.array_equal(G.jacobi(low)[0], G.jacobi(np.triu(low) + np.triu(low, 1).T)[0])


def _longdouble_moments(s):
    o = s.astype(np.longdouble)
    mu = o.mean(1)
    d = o - mu[:, None]
    return mu, (d @ d.T) / o.shape[1]


@pytest.mark.parametrize("method", ["mkl", "meanstd"])
def test_linear_maps_reach_the_palette_moments(method):
    """The mapped set's mean and covariance (for meanstd: its variances) equal the palette's.  The moments of the mapped set are taken in
    np.longdouble, so that the measurement adds nothing.  Bound: the map applies Sigma_s^(-1/2), whose condition is sqrt(kappa) with kappa
    the eigenvalue ratio of Sigma_s (at most 1e4 on these sets), twice, to numbers known to a few 2^-53: 16 kappa 2^-53 relative for mkl,
    and 16 * 4 * 2^-53 for meanstd, which touches no eigenvector.  Measured: 1.4e-13 (mkl, bound 7.8e-12 at kappa 4.4e3), 3.8e-16 (meanstd)."""
    worst = 0.0
    for seed in range(6):
        s = CASES.point_set(5000, seed)
        p = CASES.point_set(3000, 100 + seed, cond=1e-2)
        ms, mt = G.moments(s), G.moments(p)
        ev = np.linalg.eigvalsh(ms[1])
        assert ev[0] >= 1e-4 * ev[2]
        kappa = ev[2] / ev[0] if method == "mkl" else 4.0
        mu, cov = _longdouble_moments(G.linear_apply(s, ms, mt, method))
        if method == "meanstd":
            cov, want = np.diag(cov), np.diag(mt[1])
        else:
            want = mt[1]
        res = max(float(np.abs(mu - mt[0]).max() / np.abs(mt[0]).max()), float(np.abs(cov - want).max() / np.abs(want).max()))
        print(f"{method} seed {seed}: residual {res:.3e}, bound {16 * kappa * 2.0 ** -53:.3e}")
        assert res <= 16 * kappa * 2.0 ** -53
        worst = max(worst, res)
    assert worst > 0.0


@pytest.mark.parametrize("method", ["mkl", "meanstd"])
def test_linear_maps_at_the_floor(method):
    mt = G.moments(np.ascontiguousarray(CC.palettes(1, 500, seed=5)[0].T))
    flat = np.broadcast_to(np.array([[0.1], [0.7], [0.3]]), (3, 777)).copy()
    out = G.linear_apply(flat, G.moments(flat), mt, method)
    assert np.abs(out - mt[0][:, None]).max() < 1e-9                           # a flat image goes to the palette's mean
    one = np.array([[0.25], [0.5], [0.75]])                                    # n = 1: Sigma_s = 0 exactly
    m1 = G.moments(one)
    assert np.array_equal(m1[0], one[:, 0]) and not m1[1].any()
    assert np.isfinite(G.linear_apply(one, m1, mt, method)).all()
    s = CASES.point_set(300, 9)
    out = G.linear_apply(s, G.moments(s), m1, method)                          # P = 1: Sigma_t = 0, everything goes to the one point
    assert np.isfinite(out).all() and np.abs(out - one).max() < 1e-12


def test_restated_transfer_defaults_are_the_colour_reference():
    import _colour_ref as CR
    from wu import colour, paired
    x = CC.images(2, 6, 5, 1)
    pal = CC.palettes(2, 40, 2)
    rots = colour.draw_rotations(0, 2)
    mapping = paired.range_mapping((-1, 1))
    assert np.array_equal(G.transfer(x, pal, [1, 0], rots, 1.0, (-1, 1), mapping, "float32"),
                          CR.transfer(x, pal, [1, 0], rots, 1.0, (-1, 1), mapping, "float32"))
    got = G.transfer(x, pal, [1], rots, 1.0, (-1, 1), mapping, "float32", "mkl", dict(iters=(3,)))
    assert got.shape == (1, 2, 3, 6, 5) and not np.array_equal(got, G.transfer(x, pal, [1], rots, 1.0, (-1, 1), mapping, "float32", "mkl"))


def test_new_argument_errors():
    from wu import colour
    x = torch.zeros(1, 3, 4, 4)
    pal = colour.ClassPalettes(CC.palettes(2, 8, seed=1))
    for bad in ("", "IDT", "reinhard", None, 1):
        with pytest.raises(ValueError, match="method"):
            colour.transfer(x, pal, [0], method=bad)
        with pytest.raises(ValueError, match="method"):
            colour.ColourBaseline(pal, method=bad)
    for bad in ("yes", 1, (4, 16), {"iters": (4,)}):
        with pytest.raises(ValueError, match="regrain"):
            colour.transfer(x, pal, [0], regrain=bad)
        with pytest.raises(ValueError, match="regrain"):
            colour.ColourBaseline(pal, regrain=bad)
    for kw in (dict(iters=()), dict(iters=(1,) * 7), dict(iters=(4, 0)), dict(iters=(4, -1)), dict(iters=(2.5,)), dict(iters=5), dict(iters=(True,)),
               dict(smoothness=0.0), dict(smoothness=-1.0), dict(smoothness=float("inf")), dict(smoothness=float("nan")),
               dict(min_side=-1), dict(min_side=1.5)):
        with pytest.raises(ValueError, match="Regrain"):
            colour.Regrain(**kw)
        with pytest.raises(ValueError, match="Regrain"):
            colour.regrain(x, x, **kw)
    rg = colour.Regrain((2, 3), 0.5, 0)
    assert (rg.iters, rg.smoothness, rg.min_side) == ((2, 3), 0.5, 0) and colour.Regrain().iters == G.DEFAULT_ITERS
    # good new arguments on a CPU tensor get as far as the existing device check, the order of the existing checks unchanged
    for kw in (dict(method="mkl"), dict(method="meanstd", regrain=True), dict(regrain=rg), dict(regrain=None), dict(regrain=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            colour.transfer(x, pal, [0], **kw)
    with pytest.raises(ValueError, match="iters"):
        colour.transfer(x, pal, [0], iters=0, method="bad")                   # an existing check still comes first
    with pytest.raises(ValueError, match="targets"):
        colour.transfer(x, pal, [2], method="mkl")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        colour.regrain(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        colour.ColourBaseline(pal, method="mkl", regrain=True).sweep(x, torch.eye(2))
    for bad in (torch.zeros(3, 4, 4), torch.zeros(1, 4, 4, 4), np.zeros((1, 3, 4, 4))):
        with pytest.raises(ValueError, match="original"):
            colour.regrain(bad, x)
    for bad in (torch.zeros(1, 3, 4, 5), torch.zeros(2, 3, 4, 4), torch.zeros(2, 2, 3, 4, 4), torch.zeros(3, 4, 4)):
        with pytest.raises(ValueError, match="transferred"):
            colour.regrain(x, bad)
    with pytest.raises(ValueError, match="float32, bfloat16 or uint8"):
        colour.regrain(x, x.double())
    with pytest.raises(ValueError, match="max_images"):
        colour.regrain(x, x, max_images=0)
    with pytest.raises(ValueError):
        colour.regrain(x, x, value_range=(1, 1))


def test_command_line_refuses_bad_options(capsys):
    from wu import colour
    for extra in (["--method", "reinhard"], ["--regrain-smoothness", "0"], ["--regrain-smoothness", "-2"]):
        with pytest.raises(SystemExit):
            colour.main(["src", "out", "--palettes", "p.npz"] + extra)
    capsys.readouterr()
