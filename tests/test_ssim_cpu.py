"""CPU: the numpy restatement of SSIM / MS-SSIM / PSNR (tests/_ssim_ref.py) against an independent float64 torch composition, its exact
properties, the host side of wu.paired and the argument checks of wu_ssim_pairs -- nothing here launches a kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ssim_cases as CASES
import _ssim_ref as R


def _torch_composition(x, y, g, c1, c2, levels):
    """conv2d with the window as a column and then as a row, avg_pool2d(padding=[H % 2, W % 2]); mapped float64 (B, C, H, W) tensors."""
    c = x.shape[1]
    col = torch.from_numpy(g).view(1, 1, -1, 1).repeat(c, 1, 1, 1)
    row = torch.from_numpy(g).view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    filt = lambda v: F.conv2d(F.conv2d(v, col, groups=c), row, groups=c)
    out = []
    for l in range(levels):
        mux, muy = filt(x), filt(y)
        sx, sy, sxy = filt(x * x) - mux * mux, filt(y * y) - muy * muy, filt(x * y) - mux * muy
        cs = (2 * sxy + c2) / (sx + sy + c2)
        out.append(((2 * mux * muy + c1) / (mux * mux + muy * muy + c1) * cs, cs))
        if l + 1 < levels:
            pad = [x.shape[2] % 2, x.shape[3] % 2]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)      # count_include_pad: the divisor is always 4
    return out


@functools.lru_cache(maxsize=None)
def _case(h, w, k, levels):
    # Two float64 evaluations of sx, sy, sxy differ by a few 2^-53 (the terms are at most 1); the quotients magnify that by
    # 1 / ((sx + sy) + C2), up to 1 / C2 = 1100 on flat ground.  The 1e-13 below is a bound for textured pictures: noise of amplitude 0.7
    # keeps (sx + sy) + C2 above 1e-2 under every window, so two correct evaluations stay below about 1e-14 x a few.
    x, y = CASES.pair((2, 3, h, w), seed=h * 1000 + w + k, texture=0.7)
    return x, y, R.pair_stats(x, y, win_size=k, levels=levels)


@pytest.mark.parametrize("h,w,k,levels", [(33, 35, 3, 5), (33, 35, 11, 1), (224, 224, 3, 5), (224, 224, 11, 5)])
def test_restatement_against_torch_composition(h, w, k, levels):
    x, y, st = _case(h, w, k, levels)
    g = R.gaussian_window(k)
    xm, ym = (torch.from_numpy(R.mapped(v, 0.5, 0.5)) for v in (x, y))
    comp = _torch_composition(xm, ym, g, 1e-4, 9e-4, levels)
    for name, got, want in (("ssim", st["ssim_map"], comp[0][0]), ("cs", st["cs_map"], comp[0][1])):
        err = np.abs(got - want.numpy()).max()
        print(f"{h}x{w} k {k}: level-0 {name} map max |diff| {err:.2e}")
        assert err <= 1e-13
    for l in range(levels):
        assert tuple(comp[l][0].shape[2:]) == tuple(s - k + 1 for s in R.pooled_sizes(h, w, levels)[l])
        assert np.abs(st["ssim_mean"][..., l] - comp[l][0].mean((2, 3)).numpy()).max() <= 1e-13
        assert np.abs(st["cs_mean"][..., l] - comp[l][1].mean((2, 3)).numpy()).max() <= 1e-13
    if levels == 5:
        v = torch.stack([comp[l][1].mean((2, 3)) for l in range(4)] + [comp[4][0].mean((2, 3))], -1).clamp(min=0)
        want = (v ** torch.tensor(R.MS_WEIGHTS, dtype=torch.float64)).prod(-1).mean(-1).numpy()
        err = np.abs(R.combine_ms_ssim(st) - want).max()
        print(f"{h}x{w} k {k}: MS-SSIM {R.combine_ms_ssim(st)} max |diff| {err:.2e}")
        assert err <= 1e-12
        assert np.all(R.combine_ms_ssim(st) > 0.05) and np.all(R.combine_ms_ssim(st) < 0.999)      # a real value, not a degenerate one


def test_filter_against_direct_2d_sum():
    """The separable filter is the 2-D Gaussian: against the k x k double sum, to a few ulp."""
    rng = np.random.RandomState(0)
    v, g = rng.rand(20, 23), R.gaussian_window(5)
    want = sum(g[a] * g[b] * v[a:a + 16, b:b + 19] for a in range(5) for b in range(5))
    assert np.abs(R.filter_valid(v, g) - want).max() <= 16 * R.U


@pytest.mark.parametrize("k,levels,size", [(11, 1, 40), (3, 5, 40), (11, 5, 161)])
def test_identical_images_give_exactly_one(k, levels, size):
    x, _ = CASES.pair((1, 3, size, size + 1), seed=5)
    st = R.pair_stats(x, x.copy(), win_size=k, levels=levels)
    assert np.all(st["ssim_map"] == 1.0) and np.all(st["cs_map"] == 1.0)
    assert np.all(st["ssim_mean"] == 1.0) and np.all(st["cs_mean"] == 1.0)
    assert np.all(st["sse"] == 0.0) and np.all(st["sae"] == 0.0) and np.all(np.isposinf(R.psnr(st)))
    assert np.all(R.combine_ssim(st) == 1.0)
    if levels == 5:
        assert np.abs(R.combine_ms_ssim(st) - 1.0).max() <= 4 * R.U      # the weights sum to 1.0001: 1 ** w is exact, the product too


def test_negated_image_decides_the_clamp():
    """y = 1 - x: negative structure at the fine levels.  The product of clamped powers is exactly 0, where the unclamped one would be nan."""
    x = np.random.RandomState(6).rand(1, 1, 40, 40).astype(np.float32)         # cs means -0.99, -0.94, -0.83, -0.22, then ssim 0.98
    st = R.pair_stats(x, 1.0 - x, value_range=(0, 1), win_size=3, levels=5)
    cs = st["cs_mean"][0, 0]
    print("cs means of y = 1 - x:", cs)
    assert np.all(cs[:4] < 0) and cs[0] < -0.9
    assert R.combine_ms_ssim(st)[0] == 0.0
    assert R.combine_ssim(st)[0] < 0 and R.combine_ssim(st, nonnegative=True)[0] == 0.0


@pytest.mark.parametrize("a,b", [(0.25, 0.75), (0.0, 1.0), (0.6, 0.6)])
def test_constant_images(a, b):
    x, y = np.full((1, 2, 16, 17), a, np.float32), np.full((1, 2, 16, 17), b, np.float32)
    st = R.pair_stats(x, y, value_range=(0, 1), win_size=7)
    want = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)
    assert np.abs(R.combine_ssim(st) - want).max() <= 1e-9
    assert abs(R.mse(st)[0] - (a - b) ** 2) <= 1e-15 and abs(R.mae(st)[0] - abs(a - b)) <= 1e-15


def test_uint8_range_and_errors():
    x, y = CASES.pair_u8((2, 3, 20, 24), seed=3, rows=2)
    st = R.pair_stats(x, y, value_range="uint8", win_size=5)
    d = x.astype(np.int64) - y.astype(np.int64)
    assert np.array_equal(st["sse"], (d * d).sum(axis=(-3, -2, -1))) and np.array_equal(st["sae"], np.abs(d).sum(axis=(-3, -2, -1)))
    assert st["L"] == 255.0 and st["ssim_mean"].shape == (2, 2, 3, 1)
    # the same pictures as floats in (0, 1): SSIM is invariant under the common scale up to rounding
    st01 = R.pair_stats(x / np.float64(255), y / np.float64(255), value_range=(0, 1), win_size=5)
    assert np.abs(st01["ssim_mean"] - st["ssim_mean"]).max() <= 1e-10
    assert np.abs(R.psnr(st01) - R.psnr(st)).max() <= 1e-9


def test_pooled_sizes_and_front_padding():
    for s, want in CASES.POOLED.items():
        assert [h for h, _ in R.pooled_sizes(s, s)] == want
    v = np.arange(15, dtype=np.float64).reshape(3, 5)
    got = R.pool(v)
    assert got.shape == (2, 3)
    assert got[0, 0] == v[0, 0] * 0.25 and got[0, 1] == (v[0, 1] + v[0, 2]) * 0.25           # the zero row and column are in front
    assert got[1, 2] == ((v[1, 3] + v[1, 4]) + (v[2, 3] + v[2, 4])) * 0.25
    want = F.avg_pool2d(torch.from_numpy(v)[None, None], 2, padding=[1, 1])[0, 0].numpy()
    assert np.abs(got - want).max() <= 1e-15
    with pytest.raises(ValueError, match="MS-SSIM"):
        R.pair_stats(np.zeros((1, 1, 160, 200), np.float32), np.zeros((1, 1, 160, 200), np.float32), levels=5)


def test_wu_paired_host_side():
    """The window has the restatement's bits; the combinations agree with it on the restatement's own means; sizes and devices are checked."""
    from wu import paired
    for k in (3, 5, 7, 9, 11):
        assert paired.gaussian_window(k).tobytes() == R.gaussian_window(k).tobytes()
    for bad in (4, 1, 13, 2.5):
        with pytest.raises(ValueError, match="odd"):
            paired.gaussian_window(bad)
    assert paired.range_mapping((-1, 1)) == R.range_mapping((-1, 1)) == (0.5, 0.5, 1.0)
    assert paired.range_mapping((0, 1))[:1] + paired.range_mapping("uint8") == (1.0, 1.0, 0.0, 255.0)
    assert paired.MS_WEIGHTS == R.MS_WEIGHTS
    _, _, st = _case(33, 35, 3, 5)
    stats = paired.PairStats(torch.from_numpy(st["ssim_mean"]), torch.from_numpy(st["cs_mean"]),
                             torch.from_numpy(np.stack([st["sse"], st["sae"]], -1)), None, st["numel"], st["L"])
    assert np.array_equal(paired.combine_ssim(stats).numpy(), R.combine_ssim(st))
    assert np.abs(paired.combine_ms_ssim(stats).numpy() - R.combine_ms_ssim(st)).max() <= 1e-14
    assert np.abs(paired.psnr_of(stats).numpy() - R.psnr(st)).max() <= 1e-12 and np.array_equal(paired.mae_of(stats).numpy(), R.mae(st))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        paired.ssim(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="MS-SSIM"):
        paired.check_ms_size(160, 300, 11, 5)
    paired.check_ms_size(161, 300, 11, 5)
    paired.check_ms_size(12, 12, 11, 1)


def test_pair_files(tmp_path):
    from wu import paired
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    for d, names in ((a, ("p.png", "q.jpg", "only_a.png", "notes.txt")), (b, ("p.jpg", "q.png", "only_b.jpeg"))):
        for n in names:
            (d / n).write_bytes(b"")
    with pytest.raises(ValueError) as e:
        paired.pair_files(str(a), str(b))
    assert "only_a.png" in str(e.value) and "only_b.jpeg" in str(e.value) and "notes.txt" not in str(e.value)
    (a / "only_a.png").unlink(), (b / "only_b.jpeg").unlink()
    pairs = paired.pair_files(str(a), str(b))
    assert [(p.split("/")[-1], q.split("/")[-1]) for p, q in pairs] == [("p.png", "p.jpg"), ("q.jpg", "q.png")]
    (a / "p.jpg").write_bytes(b"")
    with pytest.raises(ValueError, match="stem"):
        paired.pair_files(str(a), str(b))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .jpg"):
        paired.pair_files(str(tmp_path / "empty"), str(tmp_path / "empty"))


def test_abi_argument_errors_without_a_gpu():
    """wu_ssim_pairs validates on the host before any launch; wu_ssim_workspace_bytes is 0 for anything out of range."""
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_ssim_tile_h() >= 8 and lib.wu_ssim_tile_w() >= 8
    win = (ctypes.c_double * 11)(*R.gaussian_window(11).tolist())
    one = ctypes.create_string_buffer(64)          # a non-NULL pointer; no valid call is made here
    p = ctypes.addressof(one)

    def call(dtype=0, B=1, R_=1, C=1, H=32, W=32, k=11, levels=1, x=p, ws=p):
        return lib.wu_ssim_pairs(x, 0, 0, 0, 0, p, 0, 0, 0, 0, 0, dtype, B, R_, C, H, W, 0.5, 0.5, 1.0, 0.01, 0.03, win, k, levels,
                                 ws, p, p, p, None, None)

    for kw, word in ((dict(k=4), b"odd"), (dict(k=13), b"odd"), (dict(k=1), b"odd"), (dict(H=10), b"smaller"), (dict(W=5, k=7), b"smaller"),
                     (dict(H=160, W=400, levels=5), b"MS-SSIM"), (dict(H=33, W=32, k=3, levels=5), b"MS-SSIM"), (dict(levels=3), b"levels"),
                     (dict(dtype=3), b"dtype"), (dict(x=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(B=0), b"at least 1")):
        rc = call(**kw)
        assert rc < 0 and word in lib.wu_last_error(), (kw, lib.wu_last_error())
    ws = lib.wu_ssim_workspace_bytes
    assert ws(2, 3, 3, 224, 224, 11, 5) > 0 and ws(1, 1, 1, 11, 11, 11, 1) > 0 and ws(1, 1, 1, 33, 33, 3, 5) > 0
    for bad in ((2, 3, 3, 224, 224, 10, 5), (2, 3, 3, 224, 224, 13, 1), (2, 3, 3, 160, 224, 11, 5), (2, 3, 3, 10, 224, 11, 1),
                (0, 3, 3, 224, 224, 11, 1), (2, 0, 3, 224, 224, 11, 1), (2, 3, 0, 224, 224, 11, 1), (2, 3, 3, 224, 224, 11, 2),
                (2, 3, 3, 1 << 16, 224, 11, 1)):
        assert ws(*bad) == 0, bad
    # the pooled pyramids of x and y, and two doubles per (r, n, c, tile, wave of 4) per level plus two for the errors at level 0
    th, tw = lib.wu_ssim_tile_h(), lib.wu_ssim_tile_w()
    doubles = 0
    for l, (h, w) in enumerate(R.pooled_sizes(224, 224)):
        tiles = -(-(h - 10) // th) * -(-(w - 10) // tw)
        doubles += (2 * 3 * (1 + 3) * h * w if l else 0) + 3 * 2 * 3 * tiles * 4 * 2 * (2 if l == 0 else 1)
    assert ws(2, 3, 3, 224, 224, 11, 5) == 8 * doubles
