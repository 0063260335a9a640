"""CPU: what tests/_guided_ref.py means, so that the GPU tests (tests/test_gpu_guided.py) pin the right arithmetic -- and the parts of the
guided-filter ABI that work without a GPU (argument errors, workspace size, header and binding)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _guided_cases as CASES
import _guided_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wu_guided_coeffs", "wu_guided_apply", "wu_guided_workspace_bytes", "wu_guided_tile_h", "wu_guided_tile_w")

# what the restatement gives for test_affine_target_comes_back on the CPU (32 x 40 guide, r = 3, 97 x 131 photograph)
AFFINE_OBSERVED = {1e-4: 5.63e-3, 1e-6: 5.77e-5}
# and for test_constant_target_comes_back
CONSTANT_OBSERVED = 7.8e-16


def _affine_setup():
    g = CASES.guide(1, 32, 40, 5)
    I = g.astype(np.float64) * 0.5 + 0.5
    M = np.array([[0.5, 0.2, 0.1], [0.1, 0.6, 0.1], [0.0, 0.3, 0.5]])
    off = np.array([0.05, 0.1, 0.02])
    p = (np.einsum("ck,nkhw->nchw", M, I) + off[None, :, None, None]).astype(np.float32)[None]
    photo = CASES.photo_batch([(97, 131)], 3)[0]
    want = np.einsum("ck,hwk->chw", M, photo.astype(np.float64) / 255.0) + off[:, None, None]
    return g, p, photo, want


def test_affine_target_comes_back():
    """A target that is an affine function of the guide comes back as that function of the photograph; the regulariser shrinks A by about
    eps / (variance + eps), so the error shrinks with eps.  Largest |q - want| the restatement gives here: 5.63e-3 at eps = 1e-4 and
    5.77e-5 at eps = 1e-6 (AFFINE_OBSERVED); the bound is 8 x that."""
    g, p, photo, want = _affine_setup()
    err = {}
    for eps in (1e-4, 1e-6):
        q = R.apply_one(R.coefficients(g, p, 3, eps)[0, 0], photo)
        err[eps] = np.abs(q - want).max()
        print(f"eps {eps:g}: max |q - affine(photo)| {err[eps]:.3e} (recorded {AFFINE_OBSERVED[eps]:.2e})")
        assert err[eps] <= 8 * AFFINE_OBSERVED[eps]
    assert err[1e-6] < err[1e-4]


def test_constant_target_comes_back():
    """cov = 0 up to rounding, so a = 0 and b = the constant: the deviation is rounding only (7.8e-16 here, CONSTANT_OBSERVED), not exactly
    zero: box(I p) and mI box(p) round differently."""
    g = CASES.guide(1, 32, 40, 5)
    p = np.full((1, 1, 3, 32, 40), 0.37, dtype=np.float32)
    q = R.apply_one(R.coefficients(g, p, 3, 1e-3)[0, 0], CASES.photo_batch([(97, 131)], 3)[0])
    dev = np.abs(q - np.float64(np.float32(0.37))).max()
    print(f"constant target: max deviation {dev:.3e} (recorded {CONSTANT_OBSERVED:.1e})")
    assert dev <= 8 * CONSTANT_OBSERVED


def test_equal_sizes_give_exact_taps():
    """h == hl: v = (P + 0.5) * 1 - 0.5 = P exactly, so the weights are exactly 0 and the taps the pixel itself: the plain guided filter."""
    for n in (1, 7, 32, 161):
        i0, i1, f = R.taps(n, n)
        assert np.array_equal(i0, np.arange(n)) and np.all(f == 0.0) and np.array_equal(i1, np.minimum(np.arange(n) + 1, n - 1))
    co = np.random.RandomState(0).rand(12, 7, 5)
    photo = CASES.photo_batch([(7, 5)], 1)[0]
    I = photo.astype(np.float64).transpose(2, 0, 1) / 255.0
    want = np.stack([((co[3 * c] * I[0] + co[3 * c + 1] * I[1]) + co[3 * c + 2] * I[2]) + co[9 + c] for c in range(3)])
    assert np.array_equal(R.apply_one(co, photo), want)


def test_taps_stay_inside_and_are_monotone():
    for n_full, n_low in ((1, 1), (200, 5), (131, 40), (9, 32), (1, 32), (70, 9)):
        i0, i1, f = R.taps(n_full, n_low)
        assert i0.min() >= 0 and i1.max() <= n_low - 1 and np.all(i1 >= i0) and np.all(f >= 0) and np.all(f < 1)
        assert np.all(np.diff(i0) >= 0) and np.all(np.diff(i1) >= 0)


def test_window_counts_at_the_borders():
    assert R.window_counts(7, 0).tolist() == [1] * 7
    assert R.window_counts(7, 1).tolist() == [2, 3, 3, 3, 3, 3, 2]
    assert R.window_counts(7, 3).tolist() == [4, 5, 6, 7, 6, 5, 4]
    assert R.window_counts(5, 9).tolist() == [5] * 5
    assert R.window_counts(1, 4).tolist() == [1]
    # box of ones is exactly one, box of an image with r >= size is its mean in the stated order
    assert np.all(R.box(np.ones((7, 5)), 3) == 1.0)
    v = np.random.RandomState(1).rand(4, 3)
    rows = [(v[y, 0] + v[y, 1]) + v[y, 2] for y in range(4)]
    assert np.all(R.box(v, 9) == (((rows[0] + rows[1]) + rows[2]) + rows[3]) / 12.0)
    # a corner of r = 1: two rows of two taps
    assert R.box(v, 1)[0, 0] == ((v[0, 0] + v[0, 1]) + (v[1, 0] + v[1, 1])) / 4.0


def test_global_radius_is_one_regression():
    """r >= max(hl, wl): every window is the image, so every pixel carries the same coefficients."""
    case = dict(hl=7, wl=5, rows=1, n=1)
    g, p = CASES.case_inputs(case, 4)
    co = R.coefficients(g, p, 7, 1e-3)
    assert np.all(co == co[..., :1, :1]) and np.array_equal(co, R.coefficients(g, p, 50, 1e-3))


def test_bytes_truncate():
    q = np.array([-0.1, 0.0, 0.999 / 255, 1.0 / 255, 0.5, 254.999 / 255, 1.0, 1.7])
    assert R.to_bytes(q).tolist() == [0, 0, 0, 1, 127, 254, 255, 255]


def test_new_entries_in_header_and_binding():
    from wu import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wu_kernels.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wu_[a-z0-9_]+)\s*\(", src))
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name)


def test_workspace_bytes_and_tiles_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_guided_tile_h() >= 1 and lib.wu_guided_tile_w() >= 1
    # N 9 + N 9 guide maps and R N 12 row maps of hl wl doubles
    assert lib.wu_guided_workspace_bytes(2, 3, 7, 5) == (2 * 18 + 3 * 2 * 12) * 35 * 8
    assert lib.wu_guided_workspace_bytes(1, 1, 1, 1) == 30 * 8
    for bad in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 1 << 20, 4)):
        assert lib.wu_guided_workspace_bytes(*bad) == 0


def test_argument_errors_without_a_gpu():
    """Every listed argument error is refused on the host with a message; no pointer is dereferenced and nothing is launched."""
    from wu import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                   # never dereferenced: validation comes first

    def coeffs(**kw):
        a = dict(guide=p, targets=p, dtype=_lib.F32, n=1, rows=1, hl=4, wl=4, r=1, eps=1e-3, ws=p, out=p)
        a.update(kw)
        return lib.wu_guided_coeffs(a["guide"], 48, 16, 4, 1, 0.5, 0.5, a["targets"], 48, 48, 16, 4, 1, a["dtype"], 1.0, 0.0, a["n"],
                                    a["rows"], a["hl"], a["wl"], a["r"], a["eps"], a["ws"], a["out"], None)

    for kw, word in ((dict(r=-1), b"radius"), (dict(eps=0.0), b"eps"), (dict(eps=-1e-3), b"eps"), (dict(hl=0), b"at least 1"),
                     (dict(n=0), b"at least 1"), (dict(rows=0), b"at least 1"), (dict(dtype=7), b"dtype"), (dict(guide=None), b"NULL"),
                     (dict(targets=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(out=None), b"NULL")):
        assert coeffs(**kw) < 0 and word in lib.wu_last_error(), (kw, lib.wu_last_error())

    def apply(sizes=((4, 4),), n=1, hmax=8, wmax=8, co=p, photos=p, host=True, dev=p, u8=p, f32=None, hl=4):
        flat = [v for s in sizes for v in s]
        arr = (ctypes.c_int * len(flat))(*flat) if host else None
        return lib.wu_guided_apply(co, n, 1, hl, 4, photos, hmax, wmax, arr, dev, u8, f32, None)

    for kw, word in ((dict(sizes=((9, 4),)), b"beyond"), (dict(sizes=((4, 9),)), b"beyond"), (dict(sizes=((0, 4),)), b"zero size"),
                     (dict(n=0), b"at least 1"), (dict(hmax=0), b"at least 1"), (dict(hl=0), b"at least 1"), (dict(co=None), b"NULL"),
                     (dict(photos=None), b"NULL"), (dict(host=False), b"NULL"), (dict(dev=None), b"NULL"), (dict(u8=None), b"NULL"),
                     (dict(f32=p), b"exactly one")):
        assert apply(**kw) < 0 and word in lib.wu_last_error(), (kw, lib.wu_last_error())


def test_host_glue_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from wu.guided import GuidedUpsampler
    up = GuidedUpsampler()
    assert (up.r, up.eps) == (4, 1e-3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        up.coefficients(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        up.apply(torch.zeros(1, 12, 4, 4, dtype=torch.float64), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), [(8, 8)])
    for bad in (dict(r=-1), dict(r=1.5), dict(eps=0.0), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            GuidedUpsampler(**bad)
