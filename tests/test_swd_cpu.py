"""CPU: the numpy restatement of the sliced Wasserstein distance (tests/_swd_ref.py) against independent formulations and hand-worked
values, and the host side of wu.swd (levels, draws, argument checks).  No GPU."""
import numpy as np
import pytest

import _swd_cases as CASES
import _swd_ref as R


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("h,w", [(7, 7), (8, 12), (16, 16), (32, 48)])
def test_blur_equals_reflect_padded_5x5_loop(h, w):
    """Separable, H then W, mirrored border == np.pad(mode='reflect') and an explicit 5 x 5 loop; the two sums round differently, hence a
    bound of 1e-14 relative, not equality."""
    g = np.random.RandomState(h * 100 + w).uniform(-1, 1, (h, w))
    assert _rel(R.blur(g), R.blur_2d_loop(g)) <= 1e-14
    assert _rel(R.up(g), R.up_2d_loop(g)) <= 1e-14
    assert R.down(g).shape == ((h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(R.down(g), R.blur(g)[::2, ::2])


def test_blur_keeps_a_constant_and_up_restores_it():
    g = np.full((2, 3, 8, 10), 0.375)
    assert np.array_equal(R.blur(g), g)                   # taps are dyadic and sum to 1: exact
    assert np.array_equal(R.up(R.down(g)), g)             # even and odd phases of 2 f both sum to 1


def test_mirror_index():
    i = np.arange(-5, 12)
    assert R.mirror_index(i, 7).tolist() == [5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1]


def test_hand_worked_one_dimensional_case():
    assert R.wasserstein_1d((0, 1, 3), (5, 1, 2)) == pytest.approx(4.0 / 3.0, rel=1e-15)
    with pytest.raises(ValueError):
        R.wasserstein_1d((0, 1, 3), (5, 1))


def _draws(n, h, w, levels, p=6, ndirs=16, seed=3):
    from wu import swd
    return swd.draw(seed, levels, swd.check_levels(h, w, levels), n, p, ndirs)


def test_identical_sets_give_exactly_zero():
    x = CASES.images(3, 32, 32, 0)
    pos, dirs = _draws(3, 32, 32, 2)
    assert np.array_equal(R.swd_levels(x, x, pos, dirs, 0.5, 0.5, 2), np.zeros(2))


def test_constant_shift_moves_only_the_last_level():
    """L_l = G_l - U_l kills a constant (blur and up-sampling keep it), so only the Gaussian top level sees a shift of one set's pixels;
    there the normalisation removes it from the descriptors, but not to the last bit."""
    x, y = CASES.images(3, 32, 32, 1), CASES.images(3, 32, 32, 2)
    pos, _ = _draws(3, 32, 32, 3)
    a = R.descriptors(y, pos, 0.5, 0.5, 3)
    b = R.descriptors(y, pos, 0.5, 0.5 + 0.25, 3)          # the mapped pixels of one set shifted by a constant
    for l in range(2):
        assert np.abs(a[l].astype(np.float64) - b[l]).max() <= 8 * 2.0 ** -24        # float32 rounding of values below 2
    assert np.abs(a[2].astype(np.float64) - b[2]).min() > 0.24
    pos, dirs = _draws(3, 32, 32, 3)
    base = R.swd_levels(x, y, pos, dirs, 0.5, 0.5, 3)
    lap_x, lap_y = R.descriptors(x, pos, 0.5, 0.5, 3), b
    moved = np.array([R.sliced_wasserstein(R.normalize(p), R.normalize(q), dirs).mean() for p, q in zip(lap_x, lap_y)])
    assert np.abs(moved[:2] - base[:2]).max() <= 1e-5 * base[:2].max()


def test_normalize_zero_variance_channel_and_statistics():
    d = np.random.RandomState(4).randn(10, 147).astype(np.float32)
    d[:, 49:98] = 0.625
    mu, sigma = R.statistics(d)
    assert mu[1] == 0.625 and sigma[1] == 0.0
    dn = R.normalize(d)
    assert np.all(dn[:, 49:98] == 0) and np.isfinite(dn).all()
    m2, s2 = R.statistics(dn)
    assert abs(m2[0]) < 1e-6 and abs(s2[0] - 1) < 1e-6


def test_default_levels():
    from wu import swd
    assert [swd.default_levels(s, s) for s in (256, 224, 512)] == [5, 4, 6]
    assert swd.default_levels(224, 512) == 4 and swd.default_levels(15, 400) == 0
    assert swd.check_levels(32, 48, 2) == [(32, 48), (16, 24)]


@pytest.mark.parametrize("h,w,levels", [(30, 32, 3), (32, 36, 4),          # not divisible by 2^(levels-1)
                                        (48, 48, 4), (64, 24, 3),          # a level smaller than 7
                                        (32, 32, 0), (8, 8, 0)])           # levels < 1 (8 x 8: what default_levels gives)
def test_bad_levels_raise(h, w, levels):
    from wu import swd
    with pytest.raises(ValueError):
        swd.check_levels(h, w, levels)


def test_draw_is_reproducible_bounded_and_prefix_stable():
    from wu import swd
    shapes = swd.check_levels(32, 48, 2)
    pos, dirs = swd.draw(5, 2, shapes, 4, 9, 12)
    pos2, dirs2 = swd.draw(5, 2, shapes, 4, 9, 12)
    assert np.array_equal(pos, pos2) and np.array_equal(dirs, dirs2)
    assert pos.shape == (2, 4, 9, 2) and pos.dtype == np.int32 and dirs.shape == (12, 147) and dirs.dtype == np.float32
    for l, (hl, wl) in enumerate(shapes):
        assert pos[l, ..., 0].min() >= 3 and pos[l, ..., 0].max() <= hl - 4
        assert pos[l, ..., 1].min() >= 3 and pos[l, ..., 1].max() <= wl - 4
    assert np.abs(np.linalg.norm(dirs.astype(np.float64), axis=1) - 1).max() < 1e-6
    # the documented order: directions first, then image by image, level by level, cy then cx
    rng = np.random.RandomState(5)
    d = rng.randn(147, 12)
    assert np.array_equal(dirs, (d / np.sqrt((d * d).sum(0, keepdims=True))).astype(np.float32).T)
    assert np.array_equal(pos[0, 0, :, 0], rng.randint(3, 29, size=9)) and np.array_equal(pos[0, 0, :, 1], rng.randint(3, 45, size=9))
    # image i does not depend on how many follow, and first= continues the same sequence
    tail, _ = swd.draw(5, 2, shapes, 2, 9, 12, first=2)
    assert np.array_equal(tail, pos[:, 2:])
    assert not np.array_equal(swd.draw(6, 2, shapes, 4, 9, 12)[0], pos)
    # a seeded draw covers the whole range on a small level
    many, _ = swd.draw(0, 1, [(7, 9)], 50, 8, 1)
    assert set(many[0, ..., 0].ravel()) == {3} and set(many[0, ..., 1].ravel()) == {3, 4, 5}


def test_cpu_tensors_and_bad_arguments_raise():
    import torch
    from wu import swd
    from wu.evaluate import SlicedWasserstein
    x = torch.zeros(2, 3, 16, 16)
    pos, dirs = swd.draw(0, 1, [(16, 16)], 2, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.descriptors(x, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.normalize(torch.zeros(8, 147))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.sliced_wasserstein(torch.zeros(8, 147), torch.zeros(8, 147), dirs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.swd(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SlicedWasserstein().update(x, x)


def test_library_rejects_out_of_range_without_a_launch():
    """The workspace functions return 0 and the entry points the argument error, on the host, before anything is launched."""
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_swd_sort_block() >= 64
    assert lib.wu_swd_workspace_bytes(100, 512, 0) > 0 and lib.wu_swd_workspace_bytes(100, 512, 7) == 7 * 100 * 8
    assert lib.wu_swd_workspace_bytes(0, 512, 0) == 0 and lib.wu_swd_workspace_bytes((1 << 21) + 1, 512, 0) == 0
    assert lib.wu_swd_workspace_bytes(100, 0, 0) == 0 and lib.wu_swd_workspace_bytes(100, 4097, 0) == 0
    assert lib.wu_swd_workspace_bytes(100, 512, -1) == 0
    assert lib.wu_swd_stats_workspace_bytes(0) == 0 and lib.wu_swd_stats_workspace_bytes(5) > 0
    assert lib.wu_swd_pyramid_workspace_bytes(2, 32, 32, 2, 4) > 0 and lib.wu_swd_pyramid_workspace_bytes(2, 16, 16, 1, 4) > 0
    for bad in ((2, 32, 32, 0, 4), (2, 30, 32, 3, 4), (2, 48, 48, 4, 4), (2, 32, 32, 13, 4), (1 << 14, 32, 32, 1, 256)):
        assert lib.wu_swd_pyramid_workspace_bytes(*bad) == 0, bad
    assert lib.wu_swd_project_sort(None, 0, None, 512, 0, None, None, None) < 0 and b"m 0" in lib.wu_last_error()
    assert lib.wu_swd_project_sort(None, 10, None, 4097, 0, None, None, None) < 0 and b"ndirs" in lib.wu_last_error()
    assert lib.wu_swd_distance(None, None, (1 << 21) + 1, 4, None, None) < 0 and b"m " in lib.wu_last_error()
    assert lib.wu_swd_normalize(None, 0, None, None, None, None) < 0
    assert lib.wu_swd_descriptors(None, 0, 0, 0, 0, 0, 2, 30, 32, 1.0, 0.0, 3, None, 4, None, None, None) < 0
    assert b"levels" in lib.wu_last_error()
