"""The resampling front end (csrc/resample.hip behind wu.resample.GPUResampler) against Pillow on the ragged batches of
tests/_resample_cases.py: every filter in the 8-bit mode (Image.resize on RGB uint8) and the float mode (Image.resize on mode 'F'
channels), one call per batch of images of different sizes, the padding of the source buffer poisoned (255, noise) so that a tap that
strays out of its image shows.  Bar: BIT-EXACT, no tolerance anywhere; tests/test_resample_cpu.py holds the numpy restatement to Pillow
on the same cases.  Then float sources and strided views against the restatement, every band height against the default, the workspace
across a small and a 517-tap batch, the InceptionV3 wiring against the two-step path, and a directory of mixed sizes through wu.fid."""
import numpy as np
import pytest
import torch

import _resample_cases as C
import _resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _resampler(name, filt, mode, out, band=None):
    from wu.resample import GPUResampler
    return GPUResampler(C.BATCHES[name][0], filt, mode, out, band)


def _run(name, filt, mode, out, fill="noise", band=None, rs=None):
    host, sizes = C.padded(C.pictures(name), fill)
    got = (rs or _resampler(name, filt, mode, out, band))(torch.from_numpy(host).to(DEV), sizes)
    return got.cpu().numpy()


def _same(got, want, mode):
    """got (N, 3, oh, ow) float32 raw output; want [(oh, ow, 3)] Pillow."""
    want = np.stack(want).transpose(0, 3, 1, 2)
    if mode == "u8":
        return np.array_equal(got, want.astype(np.float32))
    return np.array_equal(C.bits(got), C.bits(want))


@pytest.mark.parametrize("filt", C.FILTERS)
@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_equals_pillow(name, filt):
    """Every batch x filter, both modes, twice: padding 255 and padding noise.  All equal Pillow, hence each other."""
    for mode in C.MODES:
        want = C.want(name, filt, mode)
        for fill in ("255", "noise"):
            got = _run(name, filt, mode, "raw", fill)
            assert got.dtype == np.float32 and got.shape == (len(want), 3) + C.BATCHES[name][0]
            assert _same(got, want, mode), f"{mode}, padding {fill}: {np.count_nonzero(got != np.stack(want).transpose(0, 3, 1, 2))} values differ"


@pytest.mark.parametrize("filt", ["bicubic", "lanczos"])
def test_epilogues(filt):
    """uint8 NHWC is Pillow's image itself; 'unit' and 'nchw' are clip / 255 and Normalize(0.5, 0.5) of Pillow's value in float32, also where
    the float mode overshoots [0, 255]."""
    name = C.OVERSHOOT[0]
    want8 = np.stack(C.want(name, filt, "u8"))
    assert np.array_equal(_run(name, filt, "u8", "nhwc_u8"), want8)
    for mode in C.MODES:
        v = np.stack(C.want(name, filt, mode)).transpose(0, 3, 1, 2)
        assert mode == "u8" or (v.min() < -1 and v.max() > 256)
        assert np.array_equal(C.bits(_run(name, filt, mode, "unit")), C.bits(R.unit(v)))
        assert np.array_equal(C.bits(_run(name, filt, mode, "nchw")), C.bits(R.normalised(v)))


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("filt", ["bicubic", "lanczos"])
def test_float_sources_equal_restatement(filt, mode):
    """fp32 in (0, 1) and (-1, 1), bf16 and channels-last sources: x * 255 (or x * 127.5 + 127.5, two roundings) in float32, quantised by
    truncation in 8-bit mode, then the same resize.  A cropped view equals the contiguous copy of the same crop."""
    from wu.resample import GPUResampler
    g = torch.Generator().manual_seed(5)
    big = torch.rand(2, 3, 45, 60, generator=g) * 1.2 - 0.1              # a little outside (0, 1): the 8-bit mode clamps
    rs = GPUResampler((16, 19), filt, mode, "raw")

    def want(x, value_range):
        out = []
        for img in x.float().numpy().transpose(0, 2, 3, 1):
            t = R.to_scale_255(img, value_range)
            out.append(R.resize(R.quantise(t) if mode == "u8" else t, (16, 19), filt, mode).astype(np.float32))
        return np.stack(out).transpose(0, 3, 1, 2)

    x = big[:, :, 3:40, 5:58]                                             # 37 x 53
    dense = x.contiguous()
    for src, vr in ((dense, (0, 1)), (dense * 2 - 1, (-1, 1)), (dense.to(torch.bfloat16), (0, 1)), (dense.to(torch.bfloat16), (-1, 1)),
                    (dense.contiguous(memory_format=torch.channels_last), (-1, 1))):
        got = rs(src.to(DEV), value_range=vr).cpu().numpy()
        assert np.array_equal(C.bits(got), C.bits(want(src, vr))), (src.dtype, src.stride(), vr)
    view = big.to(DEV)[:, :, 3:40, 5:58]
    assert not view.is_contiguous()
    assert torch.equal(rs(view), rs(view.contiguous()))
    assert np.array_equal(C.bits(rs(view).cpu().numpy()), C.bits(want(dense, (0, 1))))


@pytest.mark.parametrize("name", C.BAND_BATCHES)
def test_band_heights_give_the_same_bits(name):
    """Output heights 1, 5, 29 and 31 at forced band heights 1 and 3 and the default: the same bits, run to run too."""
    for filt in ("bicubic", "lanczos"):
        for mode in C.MODES:
            base = _run(name, filt, mode, "raw")
            assert _same(base, C.want(name, filt, mode), mode)
            assert np.array_equal(C.bits(base), C.bits(_run(name, filt, mode, "raw")))
            for band in (1, 3):
                assert np.array_equal(C.bits(base), C.bits(_run(name, filt, mode, "raw", band=band))), (filt, mode, band)


def test_workspace_reuse_across_scale_ranges():
    """One resampler object per mode: the small batch, the batch with the 128.9x down-scale (517 taps), the small batch again on the grown
    workspace.  The workspace grows once; all three equal Pillow and the first equals the third bit for bit.  (The object keeps its
    output size, so the small batch here is resized to the steep batch's 20 x 30.)"""
    from wu.resample import GPUResampler
    size = C.BATCHES[C.STEEP][0]
    for mode in C.MODES:
        rs = GPUResampler(size, "bilinear", mode, "raw")

        def run(name):
            host, sizes = C.padded(C.pictures(name), "noise")
            want = [C.pillow(a, size, "bilinear", mode) for a in C.pictures(name)]
            got = rs(torch.from_numpy(host).to(DEV), sizes).cpu().numpy()
            assert _same(got, want, mode), (name, mode)
            return got

        first = run(C.SMALL)
        ws1 = rs._ws
        run(C.STEEP)
        ws2 = rs._ws
        third = run(C.SMALL)
        assert ws2 is not ws1 and ws2.numel() > ws1.numel() and rs._ws is ws2 and rs.workspace_growths == 2
        assert np.array_equal(C.bits(first), C.bits(third))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_inception_clean_equals_two_steps(prec):
    """InceptionV3(resize="clean").prepare(ragged batch, sizes=...) equals, bit for bit, the resampler to fp32 NCHW clip / 255 followed by
    InceptionV3(resize_input=False).prepare: the fused epilogue writes the network input the 299 x 299 fp32 picture would have given."""
    from wu.inception import InceptionV3
    from wu.resample import GPUResampler
    host, sizes = C.padded(C.pictures("photo_29") + C.pictures("up_29x31"), "noise")
    batch = torch.from_numpy(host).to(DEV)
    unit = GPUResampler(299, "bicubic", "f32", "unit")(batch, sizes)
    assert unit.shape == (5, 3, 299, 299) and float(unit.min()) == 0.0 and float(unit.max()) == 1.0
    for normalize in (True, False):
        fused = InceptionV3(resize="clean", precision=prec, normalize_input=normalize).prepare(batch, sizes=sizes)
        two = InceptionV3(resize_input=False, precision=prec, normalize_input=normalize).prepare(unit)
        assert fused.shape == two.shape == (5, 16, 299, 299) and fused.dtype == two.dtype and fused.stride() == two.stride()
        a, b = fused.contiguous().view(torch.int16 if prec == "bf16" else torch.int32), two.contiguous().view(torch.int16 if prec == "bf16" else torch.int32)
        assert torch.equal(a, b), normalize
    with pytest.raises(ValueError, match="resize='clean'"):
        InceptionV3(precision=prec).prepare(batch, sizes=sizes)


def test_legacy_prepare_is_unchanged_by_the_option():
    from wu.inception import InceptionV3
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(InceptionV3().prepare(x), InceptionV3(resize="legacy").prepare(x))
    assert not torch.equal(InceptionV3().prepare(x), InceptionV3(resize="clean").prepare(x))


def test_swd_reader_with_a_filter(tmp_path):
    """python -m wu.swd --size S --filter F reads through the resampler in 8-bit mode: with bilinear it equals the present --size path (the
    training pipeline's Pillow-exact bilinear resize) bit for bit; bicubic is Pillow's bicubic; without --size it is an error."""
    from PIL import Image
    from wu.files import read_images
    shapes = ((40, 56), (33, 20), (16, 16))
    images = [C.picture(h, w, "mixed", 90 + i) for i, (h, w) in enumerate(shapes)]
    files = []
    for i, a in enumerate(images):
        files.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(a, "RGB").save(files[-1])
    (plain, r0), = list(read_images(files, 16, False, DEV))
    (bil, r1), = list(read_images(files, 16, False, DEV, filter="bilinear"))
    assert r0 == r1 == (-1, 1) and torch.equal(plain, bil)
    (cub, _), = list(read_images(files, 16, False, DEV, filter="bicubic"))
    want = np.stack([C.pillow(a, (16, 16), "bicubic", "u8") for a in images]).transpose(0, 3, 1, 2)
    assert np.array_equal(C.bits(cub.cpu().numpy()), C.bits(R.normalised(want)))
    with pytest.raises(ValueError, match="--size"):
        list(read_images(files, None, False, DEV, filter="bicubic"))


def test_directory_of_mixed_sizes(tmp_path):
    """Four PNGs of four sizes: the legacy rule raises on every read path; the clean rule gives finite statistics and four rows, the same on
    the Pillow, --gpu-decode and --gpu-decode-png paths, equal to model.forward on the four images resized one by one; statistics files
    under the two rules refuse to be compared."""
    from PIL import Image
    import _inception_ref as IR
    from wu import fid
    from wu.features import FeatureBank
    from wu.inception import InceptionV3
    from wu.resample import GPUResampler
    d = tmp_path / "mixed"
    d.mkdir()
    shapes = ((40, 56), (56, 40), (299, 299), (331, 310))
    images = [C.picture(h, w, "mixed", 70 + i) for i, (h, w) in enumerate(shapes)]
    for i, a in enumerate(images):
        Image.fromarray(a, "RGB").save(str(d / f"{i}.png"))
    sd = IR.make_params(True, seed=3)
    legacy, clean, plain = InceptionV3(), InceptionV3(resize="clean"), InceptionV3(resize_input=False)
    for m in (legacy, clean, plain):
        m.load_state_dict(sd)
    for kw in ({}, {"gpu_decode": True}, {"gpu_decode_png": True}):
        with pytest.raises(ValueError):
            fid.statistics_of_path(str(d), legacy, 4, resize="legacy", **kw)
    rs = GPUResampler(299, "bicubic", "f32", "unit")
    one_by_one = torch.cat([rs(torch.from_numpy(a[None]).to(DEV)) for a in images])
    want = plain(one_by_one)[0].reshape(4, 2048)
    banks = []
    for kw in ({}, {"gpu_decode": True}, {"gpu_decode_png": True}):
        bank = FeatureBank()
        mu, sigma = fid.statistics_of_path(str(d), clean, 4, features=bank, resize="clean", **kw)
        assert mu.shape == (2048,) and sigma.shape == (2048, 2048) and np.isfinite(mu).all() and np.isfinite(sigma).all()
        assert bank.n == 4 and bank.resize == "clean" and torch.isfinite(bank.features).all()
        assert torch.equal(bank.features, want), kw
        banks.append(bank)
    with pytest.raises(ValueError, match="resize='legacy'"):
        fid.statistics_of_path(str(d), clean, 4, resize="legacy")
    a, b = str(tmp_path / "clean.npz"), str(tmp_path / "legacy.npz")
    for path, model in ((a, clean), (b, legacy)):
        st = fid.FIDStatistics(model)
        st.update_features(banks[0].features)
        st.save_npz(path)
    assert fid.npz_resize_rule(a) == "clean" and fid.npz_resize_rule(b) == "legacy"
    with pytest.raises(ValueError, match="resize rules differ"):
        fid.calculate_fid_given_paths([a, b], None)
    fb = str(tmp_path / "rows.npz")
    banks[0].save_npz(fb)
    assert FeatureBank.load_npz(fb).resize == "clean" and fid.npz_resize_rule(fb) == "clean"
