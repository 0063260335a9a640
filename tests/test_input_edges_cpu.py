"""CPU: the arithmetic of csrc/image.hip, restated in numpy (tests/_image_ref.py), against the Pillow chain (oracle/input_ref.py) at the
edge cases of tests/_image_edge_cases.py -- 1-pixel sources and windows, S = 1, exact integer scales, a 128.9x down-scale next to
up-scales, crops flush with the last row / column, rotations by 0 / +-360 / 90 / 180 / 270 / +-10 / 45 in both orders, and the colour
jitter at the factors where a fused blend and Pillow's two-step blend part.  Everything is exact equality; the HIP kernels meet the same
cases and the same Pillow reference in tests/test_gpu_input_edges.py."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import _image_edge_cases as EC
import _image_ref as REF


def _ref(case, fill, fused=False):
    return REF.pipeline(EC.padded(case, fill), case.sizes, case.params, case.S, case.augmentation, case.train, fused)


@pytest.mark.parametrize("name", EC.ALL_CASES)
def test_restatement_equals_pillow(name):
    """Bytes and the normalised float32 tensor, with the padding of the source buffer at 255 and at noise: pins _image_ref, and with
    it the kernels' documented arithmetic, at every edge -- the transpose shortcuts Image.rotate takes at 90 / 180 / 270 included."""
    case = EC.CASES[name]
    want = EC.pillow(name)
    got, u8 = _ref(case, "255")
    assert got.dtype == np.float32 and u8.dtype == np.uint8
    assert not (msg := EC.first_difference(case, got, want)), msg
    assert np.array_equal(_ref(case, "noise")[0], got), "the padding of the source buffer reached the output"
    # the float tensor holds exactly the bytes: Normalize is one-to-one on them
    assert np.array_equal(np.stack([REF.normalize(im) for im in u8]), want)


def _host_tables(monkeypatch, pipe, src, sizes, params):
    """What GPUInputPipeline.__call__ hands to the library, captured on the CPU: (geo (N, 18) int32, ksize, rot_first, factors, order,
    calls).  The library is replaced by a recorder for the length of the call; the product's API is untouched."""
    import wu.input_pipeline as ip
    from wu import _lib
    seen = {"calls": []}

    class Recorder:
        wu_image_geo_bytes = staticmethod(lambda: 72)
        wu_image_workspace_bytes = staticmethod(lambda n, S, k: (n * 2 * S * 2 + n * 2 * S * k) * 4)

    def call(fn, *a):
        seen["calls"].append(fn)
        if fn == "wu_image_geometry":
            n, S, ksize, rot_first = a[6:10]
            seen.update(geo=np.frombuffer(ctypes.string_at(a[1], n * 72), np.int32).reshape(n, 18).copy(), ksize=ksize, rot_first=rot_first,
                        ws_ok=a[3] >= Recorder.wu_image_workspace_bytes(n, S, ksize))
        else:
            n = a[4]
            seen.update(factors=np.frombuffer(ctypes.string_at(a[1], n * 12), np.float32).reshape(n, 3).copy(),
                        order=np.frombuffer(ctypes.string_at(a[2], n * 12), np.int32).reshape(n, 3).copy())
    monkeypatch.setattr(ip, "require_cuda", lambda t, what: None)
    monkeypatch.setattr(ip, "stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "load", lambda: Recorder)
    monkeypatch.setattr(_lib, "call", call)
    pipe(torch.from_numpy(src), sizes, params)
    return seen


@pytest.mark.parametrize("name", EC.ALL_CASES)
def test_host_tables_match_the_restatement(name, monkeypatch):
    """The geo rows, ksize and op tables the product builds for a case equal the ones _image_ref.geo_rows builds (so the CPU test
    above checked the kernels' arithmetic ON the product's tables); angles 0 and +-360 take the do_rot = 0 path."""
    from wu.input_pipeline import GPUInputPipeline
    case = EC.CASES[name]
    src = EC.padded(case, "255")
    seen = _host_tables(monkeypatch, GPUInputPipeline(case.S, augmentation=case.augmentation, train=case.train), src, case.sizes, case.params)
    rot_first = case.train and case.augmentation
    geo, ksize = REF.geo_rows(src.shape, case.sizes, case.params, case.S, rot_first, case.train)
    assert np.array_equal(seen["geo"], geo) and seen["ksize"] == ksize and seen["rot_first"] == int(rot_first) and seen["ws_ok"]
    for p, row in zip(case.params, seen["geo"]):
        assert row[16] == (1 if case.train and p["angle"] not in EC.NO_ROTATION else 0), p
    jitter = any(o >= 0 for p in case.params for o in p["order"])
    assert seen["calls"] == ["wu_image_geometry"] + (["wu_image_color_jitter"] if jitter else [])
    if jitter:
        assert np.array_equal(seen["factors"], np.array([p["factors"] for p in case.params], np.float32))
        assert np.array_equal(seen["order"], np.array([p["order"] for p in case.params], np.int32))


def test_host_tables_from_random_draws(monkeypatch):
    """draw() + __call__: the rows built from the product's own draws equal the rows built from the same parameter dicts."""
    from wu.input_pipeline import GPUInputPipeline, rotate_coeffs
    sizes = [(45, 70), (10, 400), (400, 10), (1, 1), (64, 64)]
    src = np.full((len(sizes), 400, 400, 3), 255, np.uint8)
    for aug in (False, True):
        pipe = GPUInputPipeline(32, augmentation=aug, seed=4)
        twin = GPUInputPipeline(32, augmentation=aug, seed=4)
        params = twin.draw(sizes)
        seen = _host_tables(monkeypatch, pipe, src, sizes, None)           # params=None: __call__ draws
        geo, ksize = REF.geo_rows(src.shape, sizes, params, 32, aug)
        assert np.array_equal(seen["geo"], geo) and seen["ksize"] == ksize
    for angle in EC.ANGLES + (-3.3, 123.4):
        for w, h in ((53, 37), (16, 16), (33, 33), (1, 1)):
            assert REF.rotate_coeffs(angle, w, h) == rotate_coeffs(angle, w, h)


@pytest.mark.parametrize("name", EC.PREMISE_CASES)
def test_cases_tell_a_fused_blend_from_pillow(name):
    """The premise of the jitter cases: with the blend rounded ONCE (a fused multiply-add) every Contrast / Color image at a factor of
    0.8, 1.1, 1.2, 2/3 or 4/3 differs from Pillow in at least one byte; rounded twice, none does.  Brightness blends against 0: the sum
    is the product and one rounding equals two."""
    case = EC.CASES[name]
    want = EC.pillow(name)
    two_step, fused = _ref(case, "255")[0], _ref(case, "255", fused=True)[0]
    counts = {}
    for n, tag in enumerate(case.tags):
        op, f = tag
        counts[tag] = int((fused[n] != want[n]).sum())
        assert np.array_equal(two_step[n], want[n]), tag
        if op == "Brightness":
            assert counts[tag] == 0, tag
        elif f in EC.SENSITIVE:
            assert counts[tag] >= 1, f"{name}: {tag} cannot see a fused blend"
    print(name, "bytes a fused blend gets wrong:", {f"{op} {f:.4g}": c for (op, f), c in counts.items() if c})
    assert {(op, f) for (op, f), c in counts.items() if c} >= {(op, f) for op in ("Contrast", "Color") for f in EC.SENSITIVE}


def test_pillow_blend_rounds_twice():
    """Image.blend equals the two-step float32 blend for all 65,536 (degenerate, value) byte pairs at every factor of the grid -- the
    assumption the unfused kernel rests on.  A Pillow build that fused the blend would fail HERE, on the CPU.  The one-rounding blend
    differs at the sensitive factors (and only there, within the grid)."""
    d, v = np.mgrid[0:256, 0:256].astype(np.uint8)
    im_d, im_v = Image.fromarray(d, "L"), Image.fromarray(v, "L")
    wrong = {}
    for f in EC.GRID:
        want = np.asarray(Image.blend(im_d, im_v, f))
        assert np.array_equal(REF.blend8(d, v, f), want), f
        wrong[f] = int((REF.blend8(d, v, f, fused=True) != want).sum())
    print("pairs of 65536 a fused blend gets wrong:", {f"{f:.4g}": c for f, c in wrong.items()})
    assert all((wrong[f] > 0) == (f in EC.SENSITIVE) for f in EC.GRID), wrong


def test_tap_count_never_exceeds_the_images_own_ksize():
    """resample_coeffs_kernel clamps a tap count to the batch ksize.  The clamp must never bind -- it would drop taps Pillow uses:
    every count is at most the image's OWN ksize = 2 * ceil(max(in / S, 1)) + 1, which the batch ksize is the maximum of."""
    for S in (1, 2, 3, 7, 8, 16, 33, 64):
        for in_size in list(range(1, 4 * S + 3)) + [257, 1031, 4096]:
            own = REF.ksize_for(in_size, S)
            bounds, coeffs = REF.coeff_table(in_size, S, own + 2)
            assert bounds[:, 1].max() <= own and (bounds[:, 1] >= 1).all() and not coeffs[:, own:].any(), (in_size, S)
            assert (bounds[:, 0] + bounds[:, 1] <= in_size).all(), (in_size, S)
            assert (np.abs(coeffs.sum(1) - (1 << REF.PREC)) <= own).all(), (in_size, S)


@pytest.mark.parametrize("hw, want", [((10, 400), (0, 193, 10, 13)), ((400, 10), (193, 0, 13, 10))])
def test_resized_crop_falls_back_to_the_central_crop(hw, want):
    """RandomResizedCrop.get_params on a 40:1 image with scale (0.9, 1.0): no attempt fits (the short side would need >= 52 pixels), so
    the central crop with the ratio clamped to 4/3 (3/4) comes back -- inside the image, and after exactly ten attempts' worth of draws."""
    import random
    from wu.input_pipeline import GPUInputPipeline
    h, w = hw
    for seed in range(20):
        pipe = GPUInputPipeline(32, augmentation=True, seed=seed, scale=(0.9, 1.0))
        i, j, ch, cw = crop = pipe._resized_crop_params(h, w)
        assert crop == want
        assert 0 <= i and 0 <= j and ch >= 1 and cw >= 1 and i + ch <= h and j + cw <= w
        assert round(max(cw / ch, ch / cw), 1) == 1.3 and (ch == h or cw == w)
        twin = random.Random(seed)
        [twin.random() for _ in range(20)]                               # ten attempts, two uniform draws each, no randint
        assert pipe.rng.random() == twin.random()
    # and the whole draw() stays inside the image, so __call__ accepts it
    p = GPUInputPipeline(32, augmentation=True, seed=1, scale=(0.9, 1.0)).draw([hw])[0]
    assert p["crop"] == want
