"""CPU: the arithmetic of the resampling front end (wu.resample, csrc/resample.hip).  The numpy restatement (tests/_resample_ref.py) equals
Pillow's Image.resize BIT FOR BIT for the box, bilinear, bicubic and Lanczos filters, on RGB uint8 (np.array_equal) and on mode 'F'
channels (float32 bit patterns), over the ragged cases of tests/_resample_cases.py; the coefficient tables the product uploads equal the
restatement's float64 weights bit for bit; argument errors are reported on the host."""
import ctypes

import numpy as np
import pytest

import _resample_cases as C
import _resample_ref as R


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("filt", C.FILTERS)
@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_restatement_equals_pillow(name, filt, mode):
    size = C.BATCHES[name][0]
    for img, want in zip(C.pictures(name), C.want(name, filt, mode)):
        src = img if mode == "u8" else img.astype(np.float32)
        got = R.resize(src, size, filt, mode)
        assert got.shape == want.shape and got.dtype == want.dtype
        if mode == "u8":
            assert np.array_equal(got, want), f"{img.shape[:2]} -> {size}: {np.count_nonzero(got != want)} bytes differ"
        else:
            assert np.array_equal(C.bits(got), C.bits(want)), f"{img.shape[:2]} -> {size}: {np.count_nonzero(C.bits(got) != C.bits(want))} floats differ"


def test_float_mode_overshoots_and_box_does_not():
    """No clipping inside the float resize: bicubic and Lanczos leave [0, 255] on the stripe picture, box and bilinear cannot."""
    name, k = C.OVERSHOOT
    for filt in C.FILTERS:
        v = C.want(name, filt, "f32")[k]
        outside = v.min() < -1.0 and v.max() > 256.0
        assert outside == (filt in ("bicubic", "lanczos")), (filt, float(v.min()), float(v.max()))


def test_both_passes_skipped_is_the_source():
    img = C.pictures("up_29x31")[1]
    for filt in C.FILTERS:
        assert np.array_equal(R.resize(img, (29, 31), filt, "u8"), img)
        assert np.array_equal(R.resize(img.astype(np.float32), (29, 31), filt, "f32"), img.astype(np.float32))


def _axis_pairs():
    pairs = set()
    for (oh, ow), items in C.BATCHES.values():
        for h, w, _ in items:
            pairs.add((w, ow))
            pairs.add((h, oh))
    return sorted(p for p in pairs if p[0] != p[1])


@pytest.mark.parametrize("filt", C.FILTERS)
def test_product_tables_equal_restatement(filt):
    """wu.resample.coefficients (vectorised numpy; Lanczos through math.sin) against the scalar restatement: bounds, every float64 weight
    bit for bit, zeros beyond the count, and the 22-bit fixed-point form."""
    from wu import resample
    for in_size, out_size in _axis_pairs():
        bounds, kk = resample.coefficients(in_size, out_size, filt)
        ref = R.precompute_coeffs(in_size, out_size, filt)
        assert bounds.shape == (out_size, 2) and kk.shape[0] == out_size and kk.dtype == np.float64
        fixed = resample.coefficients_8bpc(kk)
        for xx, (xmin, ws) in enumerate(ref):
            assert (int(bounds[xx, 0]), int(bounds[xx, 1])) == (xmin, len(ws)), (in_size, out_size, xx)
            assert len(ws) <= kk.shape[1]
            assert np.array_equal(kk[xx, :len(ws)].view(np.uint64), np.array(ws, dtype=np.float64).view(np.uint64)), (in_size, out_size, xx)
            assert not kk[xx, len(ws):].any()
            assert fixed[xx, :len(ws)].tolist() == [R._fixed(w) for w in ws]


def test_argument_errors_without_a_gpu():
    from wu import _lib, resample
    lib = _lib.load()
    assert lib.wu_resample_desc_bytes() == resample._DESC.itemsize == 64
    assert lib.wu_resample_workspace_bytes(0, 0) == 0 and lib.wu_resample_workspace_bytes(2, 10) == 2 * 64 + 16
    one = ctypes.create_string_buffer(64)
    rc = lib.wu_resample(one, 0, one, one, 64, 1, 2000, 16, one, 0, 0, 0, 1 << 4, None)
    assert rc < 0 and b"at most 1024" in lib.wu_last_error()
    rc = lib.wu_resample(one, 0, one, one, 64, 1, 16, 16, one, 0, 0, 0, 0, None)           # uint8 output in float mode
    assert rc < 0 and b"8-bit mode" in lib.wu_last_error()
    rc = lib.wu_resample(one, 0, one, one, 64, 1, 16, 16, one, 0, 0, 0, (1 << 4) | (9 << 8), None)
    assert rc < 0 and b"band" in lib.wu_last_error()
    with pytest.raises(ValueError, match="1024"):
        resample.GPUResampler((2000, 16))
    with pytest.raises(ValueError, match="filter"):
        resample.GPUResampler(16, "hamming")
    with pytest.raises(ValueError, match="mode='u8'"):
        resample.GPUResampler(16, out="nhwc_u8")
    with pytest.raises(ValueError, match="band"):
        resample.GPUResampler(16, band=9)
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample.GPUResampler(16)(torch.zeros(1, 20, 20, 3, dtype=torch.uint8))


def test_npz_files_record_the_resize_rule(tmp_path):
    """A statistics file without the key is legacy; files under different rules refuse to be compared, before any model is loaded."""
    from wu import fid
    mu, sigma = np.zeros(4), np.eye(4)
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    np.savez(a, mu=mu, sigma=sigma)
    np.savez(b, mu=mu, sigma=sigma, resize=np.array("clean"))
    assert fid.npz_resize_rule(a) == "legacy" and fid.npz_resize_rule(b) == "clean"
    with pytest.raises(ValueError, match="resize rules differ"):
        fid.calculate_fid_given_paths([a, b], None)
    with pytest.raises(ValueError, match="resize rules differ"):
        fid.statistics_of_path(a, None, 50, resize="clean")
    assert fid.calculate_fid_given_paths([a, a], None) == pytest.approx(0.0, abs=1e-9)
    assert fid.calculate_fid_given_paths([b, b], None, resize="clean") == pytest.approx(0.0, abs=1e-9)
