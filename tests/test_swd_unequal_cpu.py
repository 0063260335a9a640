"""CPU: the closed form of the W1 distance between samples of unequal length (tests/_swd_unequal_ref.py, the rule of wu/swd.py's
"Distance" paragraph) against exact rational arithmetic over the merged breakpoints and against scipy, and the host side of
``unequal="exact"``: argument checks of the library and of wu.swd.  No GPU.

Integer keys: every weight, difference and product is an integer below 2^53, so the closed form's sum is exact in any order and its
one division rounds the exact rational once -- equal to ``float(exact)`` bit for bit.  Gaussian keys: 2 ml non-negative terms summed in
any order are off by at most (2 ml - 1) u relative, each term by 2 u (difference, product), the quotient by u: (2 ml + 8) u covers
them to first order, u = 2^-53."""
import fractions

import numpy as np
import pytest

import _swd_unequal_ref as REF

PAIRS = [(1, 2), (2, 1), (2, 3), (3, 2), (6, 4), (4, 6), (1, 257), (257, 512), (512, 257), (63, 64), (255, 256), (256, 257), (1000, 7),
         (7, 1000)]
U = fractions.Fraction(1, 2 ** 53)


def _integers(m1, m2):
    rng = np.random.RandomState(1000 * m1 + m2)
    return rng.randint(-50, 51, m1).astype(np.float64), rng.randint(-50, 51, m2).astype(np.float64)


@pytest.mark.parametrize("m1,m2", PAIRS)
def test_closed_form_equals_rationals_on_integer_keys(m1, m2):
    a, b = _integers(m1, m2)
    want = REF.exact(a, b)
    assert want > 0 and REF.closed_form(a, b) == float(want)
    assert REF.closed_form(b, a) == float(want)


@pytest.mark.parametrize("m1,m2", PAIRS)
def test_closed_form_within_the_summation_bound_on_gaussian_keys(m1, m2):
    rng = np.random.RandomState(7 * m1 + m2)
    a, b = rng.randn(m1), 0.8 * rng.randn(m2) + 0.1
    want = REF.exact(a, b)
    got = fractions.Fraction(REF.closed_form(a, b))
    rel = abs(got - want) / want
    print(f"({m1}, {m2}): relative error {float(rel):.3e}, bound {float((2 * max(m1, m2) + 8) * U):.3e}")
    assert rel <= (2 * max(m1, m2) + 8) * U


@pytest.mark.parametrize("m1,m2", PAIRS)
def test_closed_form_agrees_with_scipy(m1, m2):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.RandomState(3 * m1 + m2)
    a, b = rng.randn(m1), 0.8 * rng.randn(m2) + 0.1
    want = stats.wasserstein_distance(a, b)
    assert abs(REF.closed_form(a, b) - want) <= 1e-12 * want


@pytest.mark.parametrize("m1,m2", PAIRS)
def test_an_interval_meets_at_most_two(m1, m2):
    ml, ms = max(m1, m2), min(m1, m2)
    j0, j1, w0, w1 = REF.weights(ml, ms)
    assert np.all(j1 - j0 >= 0) and np.all(j1 - j0 <= 1) and j0[0] == 0 and j1[-1] == ms - 1
    assert np.all(w0 + w1 == ms) and np.all(w0 >= 1) and np.all((w1 == 0) == (j1 == j0))
    # every y_j is met over ml units in all
    got = np.bincount(j0, weights=w0, minlength=ms) + np.bincount(j1, weights=w1, minlength=ms)
    assert np.array_equal(got, np.full(ms, ml))


@pytest.mark.parametrize("m1,m2,k", [(6, 4, 2), (4, 6, 3), (257, 100, 2), (63, 64, 5), (7, 1, 9)])
def test_replicating_every_key_changes_no_bit(m1, m2, k):
    a, b = _integers(m1, m2)
    assert REF.closed_form(a, np.repeat(b, k)) == REF.closed_form(a, b)
    assert REF.exact(a, np.repeat(b, k)) == REF.exact(a, b)
    assert REF.closed_form(np.repeat(a, k), a) == 0.0


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_equal_counts_reduce_to_the_mean_absolute_difference(m):
    a, b = _integers(m, m)
    assert REF.closed_form(a, b) == np.abs(np.sort(a) - np.sort(b)).sum() / m


def test_hand_worked_case():
    """a = (0, 4), b = (1, 2, 6): over sixths of [0, 1], |0-1| |0-1| |0-2| |4-2| |4-6| |4-6| = 1 + 1 + 2 + 2 + 2 + 2 -> 10/6."""
    assert REF.exact((0, 4), (1, 2, 6)) == fractions.Fraction(5, 3)
    assert REF.closed_form((4, 0), (6, 1, 2)) == 10.0 / 6.0


def test_library_rejects_out_of_range_without_a_launch():
    from wu import _lib
    lib = _lib.load()
    big = (1 << 21) + 1
    for m1, m2, nd in ((0, 4, 2), (4, 0, 2), (big, 4, 2), (4, big, 2), (-1, 4, 2)):
        assert lib.wu_swd_distance_unequal(None, m1, None, m2, nd, None, None) < 0
        err = lib.wu_last_error()
        assert b"wu_swd_distance_unequal" in err and b"m1" in err
    for nd in (0, 4097):
        assert lib.wu_swd_distance_unequal(None, 4, None, 5, nd, None, None) < 0
        err = lib.wu_last_error()
        assert b"wu_swd_distance_unequal" in err and b"ndirs" in err
    assert lib.wu_swd_distance_unequal(None, 4, None, 5, 2, None, None) < 0
    assert b"wu_swd_distance_unequal: NULL pointer" in lib.wu_last_error()


def test_cpu_tensors_raise():
    import torch
    from wu import swd
    from wu.evaluate import SlicedWasserstein
    x = torch.zeros(3, 3, 16, 16)
    dirs = swd.draw(0, 1, [(16, 16)], 1, 1, 8)[1]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.sliced_wasserstein(torch.zeros(8, 147), torch.zeros(5, 147), dirs, unequal="exact")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.swd(x, x[:2], unequal="exact")
    bank = swd.DescriptorBank()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.add(x)
    with pytest.raises(RuntimeError, match="no batch"):
        swd.compare(bank, bank)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SlicedWasserstein(reference=bank).update(x, x)


def test_a_bogus_rule_raises():
    import torch
    from wu import swd
    x = torch.zeros(2, 3, 16, 16)
    dirs = swd.draw(0, 1, [(16, 16)], 1, 1, 8)[1]
    with pytest.raises(ValueError, match="bogus"):
        swd.sliced_wasserstein(torch.zeros(8, 147), torch.zeros(8, 147), dirs, unequal="bogus")
    with pytest.raises(ValueError, match="bogus"):
        swd.distances([torch.zeros(8, 147)], [torch.zeros(8, 147)], dirs, unequal="bogus")
    with pytest.raises(ValueError, match="bogus"):
        swd.swd(x, x, unequal="bogus")
    with pytest.raises(ValueError, match="bogus"):
        swd.swd_of_dirs("a", "b", unequal="bogus")
    with pytest.raises(SystemExit):
        swd.main(["a", "b", "--unequal", "bogus"])
