"""CPU: the colour-transfer baseline's host side (wu.colour) and the properties of its numpy restatement (tests/_colour_ref.py) that the
GPU tests then hold the kernels to.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import _colour_cases as CASES
import _colour_ref as R

UNIT = (1.0, 0.0, 1.0)                  # range_mapping((0, 1))


def test_draw_rotations():
    from wu import colour
    rots = colour.draw_rotations(3, 9)
    assert rots.shape == (9, 3, 3) and rots.dtype == np.float64
    assert np.array_equal(rots[0], np.eye(3))
    for k in range(9):
        assert np.abs(rots[k] @ rots[k].T - np.eye(3)).max() <= 1e-14
    assert np.array_equal(colour.draw_rotations(3, 4), rots[:4])
    assert not np.array_equal(colour.draw_rotations(4, 4)[1], rots[1])
    # the rule of the docstring, restated: R_k = (Q sign(diag T))^T of the k-th draw
    rng = np.random.RandomState(3)
    for k in range(1, 4):
        Q, T = np.linalg.qr(rng.randn(3, 3))
        assert np.array_equal(rots[k], (Q * np.sign(np.diag(T))).T)
    with pytest.raises(ValueError):
        colour.draw_rotations(0, 0)


def _argsort_match(src, ref):
    """Classic histogram matching of one channel with as many reference values as pixels: the i-th smallest pixel takes the i-th smallest
    reference value."""
    out = np.empty_like(ref)
    out[np.argsort(src, kind="stable")] = np.sort(ref)
    return out


def test_one_iteration_is_per_channel_histogram_matching():
    n = 64
    x = CASES.distinct_integer_image(n, 1)
    pal = CASES.distinct_integer_image(n, 2).reshape(3, n).T.astype(np.float64)          # (P = n, 3)
    got = R.transfer(x, pal[None], [0], np.eye(3)[None], 1.0, (0, 1), UNIT, "float32")[0, 0].reshape(3, n)
    for c in range(3):
        want = _argsort_match(x[0, c, 0].astype(np.float64), pal[:, c])
        assert np.array_equal(got[c], want.astype(np.float32))
        assert np.array_equal(np.sort(got[c]), np.sort(pal[:, c]).astype(np.float32))


@pytest.mark.parametrize("kind", ["noise", "ties", "flat"])
def test_own_pixels_as_palette_return_the_image(kind):
    from wu import colour
    x = {"noise": CASES.images(1, 5, 7, 3), "ties": CASES.two_colour(1, 5, 7, 4), "flat": CASES.flat(1, 5, 7)}[kind]
    mapping = (0.5, 0.5, 1.0)
    pal = R.load_state(x, *mapping)[0].T                                                 # (n, 3): the image's own pixels
    got = R.transfer(x, pal[None], [0], colour.draw_rotations(0, 4), 1.0, (-1, 1), mapping, "float32")
    assert np.array_equal(got[0], x)
    u = CASES.noise_u8(1, 5, 7, 5)
    pal = R.load_state(u, 1.0, 0.0, 255.0)[0].T
    assert np.array_equal(R.transfer(u, pal[None], [0], colour.draw_rotations(0, 4), 0.5, "uint8", (1.0, 0.0, 255.0), "uint8")[0], u)


def test_equal_colours_stay_equal_and_pixels_permute():
    from wu import colour
    rots = colour.draw_rotations(1, 3)
    pal = CASES.palettes(1, 50, 6)
    x = CASES.two_colour(1, 6, 9, 7)
    got = R.transfer(x, pal, [0], rots, 1.0, (-1, 1), (0.5, 0.5, 1.0), "float32")[0, 0].reshape(3, -1)
    src = x[0].reshape(3, -1)
    assert len(np.unique(src, axis=1).T) == 2 and len(np.unique(got, axis=1).T) == 2
    for col in np.unique(src, axis=1).T:
        same = (src == col[:, None]).all(0)
        assert len(np.unique(got[:, same], axis=1).T) == 1
    y = CASES.images(1, 6, 9, 8)
    perm = np.random.RandomState(9).permutation(54)
    yp = y.reshape(1, 3, 54)[:, :, perm].reshape(1, 3, 6, 9)
    a = R.transfer(y, pal, [0], rots, 1.0, (-1, 1), (0.5, 0.5, 1.0), "float32").reshape(3, 54)
    b = R.transfer(yp, pal, [0], rots, 1.0, (-1, 1), (0.5, 0.5, 1.0), "float32").reshape(3, 54)
    assert np.array_equal(a[:, perm], b)


@pytest.mark.parametrize("n,p", CASES.RANK_NP)
def test_quantile_index_stays_in_range(n, p):
    rng = np.random.RandomState(n * 31 + p)
    for keys in (rng.randn(n), np.zeros(n), rng.randint(0, 2, n).astype(np.float64), np.arange(n, dtype=np.float64)):
        t = R.ranks(keys, p)
        assert t.dtype == np.int64 and t.min() >= 0 and t.max() <= p - 1
    assert np.array_equal(R.ranks(np.arange(n, dtype=np.float64), p), ((2 * np.arange(n) + 1) * p) // (2 * n))


def test_palette_from_images_draw_order():
    from wu import colour
    x = CASES.images(3, 5, 4, 10)
    rng = np.random.RandomState(11)
    i, yy, xx = rng.randint(0, 3, 17), rng.randint(0, 5, 17), rng.randint(0, 4, 17)
    got = colour.palette_from_images(torch.from_numpy(x), 17, seed=11, value_range=(-1, 1))
    assert got.shape == (17, 3) and got.dtype == torch.float64
    assert np.array_equal(got.numpy(), (x[i, :, yy, xx].astype(np.float64) * 0.5 + 0.5) / 1.0)
    u = CASES.images_u8(3, 5, 4, 12)
    got = colour.palette_from_images(torch.from_numpy(u), 17, seed=11, value_range="uint8")
    assert np.array_equal(got.numpy(), u[i, :, yy, xx].astype(np.float64) / 255.0)
    with pytest.raises(ValueError):
        colour.palette_from_images(torch.from_numpy(x), 0)
    with pytest.raises(ValueError):
        colour.palette_from_images(torch.from_numpy(x[0]), 4)


def test_class_palettes_round_trip_and_checks(tmp_path):
    from wu import colour
    pal = colour.ClassPalettes(CASES.palettes(2, 9, 13), ["snowy", "rainy"], seed=5, sources=["a", "b"])
    assert pal.num_classes == 2 and pal.P == 9
    pal.save_npz(tmp_path / "p.npz")
    back = colour.ClassPalettes.load_npz(tmp_path / "p.npz")
    assert torch.equal(back.palettes, pal.palettes) and back.names == ["snowy", "rainy"] and back.seed == 5 and back.sources == ["a", "b"]
    bad = CASES.palettes(2, 9, 13)
    bad[1, 3, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        colour.ClassPalettes(bad)
    with pytest.raises(ValueError):
        colour.ClassPalettes(np.zeros((2, 0, 3)))
    with pytest.raises(ValueError):
        colour.ClassPalettes(np.zeros((2, 9, 4)))
    with pytest.raises(ValueError):
        colour.ClassPalettes(np.zeros((2, 9, 3)), names=["one"])


def test_sweep_rejects_rows_that_are_not_one_hot():
    from wu import colour
    base = colour.ColourBaseline(CASES.palettes(3, 9, 14), iters=2)
    assert base.eval() is base and base.train() is base and base.train(False) is base
    x = torch.zeros(2, 3, 4, 4)
    for rows in ([[0.5, 0.5, 0.0]], [[0.0, 0.0, 0.0]], [[1.0, 1.0, 0.0]], [[1.0, 0.0, 0.0], [0.0, 0.3, 0.0]], [[0.0, 2.0, 0.0]]):
        with pytest.raises(ValueError, match="one-hot"):
            base.sweep(x, torch.tensor(rows))
    with pytest.raises(ValueError):
        base.sweep(x, torch.eye(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # one-hot rows pass the check and reach transfer
        base.sweep(x, torch.eye(3))


def test_transfer_rejects_cpu_tensors_and_bad_arguments():
    from wu import colour
    pal = colour.ClassPalettes(CASES.palettes(2, 9, 15))
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        colour.transfer(x, pal, [0, 1])
    for bad in ([2], [-1], [], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            colour.transfer(x, pal, bad)
    with pytest.raises(ValueError):
        colour.transfer(x, pal, torch.tensor([0, 2]))
    with pytest.raises(ValueError):
        colour.transfer(torch.zeros(2, 4, 4, 4), pal, [0])
    with pytest.raises(ValueError):
        colour.transfer(torch.zeros(2, 3, 4), pal, [0])
    with pytest.raises(ValueError):
        colour.transfer(torch.zeros(2, 3, 4, 0), pal, [0])
    with pytest.raises(ValueError):
        colour.transfer(torch.zeros(1, 3, 1, (1 << 21) + 1, dtype=torch.uint8), pal, [0], value_range="uint8")
    with pytest.raises(ValueError):
        colour.transfer(x.double(), pal, [0])
    with pytest.raises(ValueError):
        colour.transfer(x, pal, [0], iters=0)
    with pytest.raises(ValueError):
        colour.transfer(x, pal, [0], max_images=0)
    with pytest.raises(ValueError):
        colour.transfer(x, pal, [0], value_range=(1, 1))
    with pytest.raises(ValueError, match="finite"):
        colour.transfer(x, torch.full((1, 4, 3), float("nan"), dtype=torch.float64), [0])


def test_workspace_is_zero_out_of_range():
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_colour_ot_workspace_bytes(2, 48 * 40, 3, 100) > 0
    for bad in ((0, 10, 1, 10), (1, 0, 1, 10), (1, (1 << 21) + 1, 1, 10), (1, 10, 0, 10), (1, 10, 1, 0), (1, 10, 1, (1 << 21) + 1),
                (-1, 10, 1, 10)):
        assert lib.wu_colour_ot_workspace_bytes(*bad) == 0, bad
