"""GPU: the JPEG decoder with ``coverage="extended"`` (wu/jpeg.py, csrc/jpeg_host.h, csrc/jpeg.hip): progressive files and 4:4:0
sampling decoded natively, against Pillow.  Bar: exact equality of every byte, inside each image's H x W with Pillow's decode and zero
outside it."""
import os

import numpy as np
import pytest
import torch

import _jpeg_prog_ref as P
import _jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def _check(src_u8, sizes, datas, names=None, want=None):
    out = src_u8.cpu().numpy()
    assert out.shape[0] == len(datas) and out.shape[3] == 3 and out.dtype == np.uint8
    assert out.shape[1] == max(h for h, _ in sizes) and out.shape[2] == max(w for _, w in sizes)
    for i, d in enumerate(datas):
        ref = R.pillow_rgb(d) if want is None else want[i]
        h, w = ref.shape[:2]
        name = names[i] if names else i
        assert tuple(sizes[i]) == (h, w), name
        got = out[i, :h, :w]
        assert np.array_equal(got, ref), f"{name}: {np.count_nonzero(got != ref)} of {ref.size} bytes differ, max {np.abs(got.astype(int) - ref).max()}"
        pad = out[i].copy()
        pad[:h, :w] = 0
        assert not pad.any(), f"{name}: {np.count_nonzero(pad)} non-zero padding bytes"


def test_one_mixed_batch_equals_pillow():
    from wu.jpeg import GPUJpegDecoder
    img = R.synth(97, 131, 3)
    prog420 = P.encode(img, dict(quality=75), True)
    cases = [("baseline_420", P.encode(img, dict(quality=75), False)), ("prog_420", prog420),
             ("prog_444", P.encode(R.synth(64, 48, 4), dict(quality=90, subsampling=0), True)), ("prog_grey", P.encode(R.synth(33, 17, 5), "grey", True)),
             ("s440_baseline", P.make_440(48)), ("s440_prog", P.make_440(33, progressive=True)), ("incomplete", P.make_incomplete(prog420, 5)),
             ("cmyk.jpg", _golden("cmyk.jpg")), ("rgb.png", _golden("rgb.png")), ("progressive.jpg", _golden("progressive.jpg")),
             ("s440.jpg", _golden("s440.jpg")), ("prog_422_rst", P.encode(R.synth(120, 161, 6), dict(quality=85, subsampling=1, restart_marker_blocks=3), True))]
    dec = GPUJpegDecoder(DEV, coverage="extended")
    src, sizes, status = dec.decode_batch([d for _, d in cases], return_status=True)
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    _check(src, sizes, [d for _, d in cases], [n for n, _ in cases])
    assert dec.stats == {"native": 9, "fallback": 3, "fallback_reasons": {"progressive-incomplete": 1, "colorspace": 1, "not-jpeg": 1}}
    assert status == ["ok"] * 6 + ["progressive-incomplete", "colorspace", "not-jpeg"] + ["ok"] * 3
    dec.close()
    # the default decoder on the same batch: the same bytes, the extended files through Pillow
    dec = GPUJpegDecoder(DEV)
    src0, sizes0 = dec.decode_batch([d for _, d in cases])
    assert sizes0 == sizes and torch.equal(src0, src)
    assert dec.stats["native"] == 1 and dec.stats["fallback_reasons"] == {"progressive": 7, "sampling": 2, "colorspace": 1, "not-jpeg": 1}
    dec.close()


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (8, 8), (33, 17), (3, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_progressive_edge_sizes_one_image_per_batch(size):
    from wu.jpeg import GPUJpegDecoder
    dec = GPUJpegDecoder(DEV, threads=2, coverage="extended")
    for name, prog, _ in P.twins(size, 7):
        src, sizes = dec.decode_batch([prog])
        assert tuple(src.shape) == (1, size[0], size[1], 3)
        _check(src, sizes, [prog], [name])
    assert dec.stats["fallback"] == 0 and dec.stats["native"] == len(P.PROG_VARIANTS)
    dec.close()


@pytest.mark.parametrize("side", [1, 16, 17])
def test_440_edge_sizes_one_image_per_batch(side):
    """One chroma row (1); whole MCUs of 8 x 16 luma (16: two across, one down); an odd height past an MCU row, whose last chroma row
    has no row below it (17)."""
    from wu.jpeg import GPUJpegDecoder
    dec = GPUJpegDecoder(DEV, threads=2, coverage="extended")
    for progressive in (False, True):
        data = P.make_440(side, seed=side, progressive=progressive)
        src, sizes = dec.decode_batch([data])
        assert tuple(src.shape) == (1, side, side, 3)
        _check(src, sizes, [data], [f"440_{side}_{progressive}"])
    assert dec.stats == {"native": 2, "fallback": 0, "fallback_reasons": {}}
    dec.close()


def test_device_kernels_alone_equal_the_numpy_restatement_h1v2():
    """wu_jpeg_reconstruct in WU_JPEG_MODE_H1V2 on coefficients uploaded by the test itself, against the numpy restatement on the SAME
    coefficients, beside a 4:2:0 image in the same batch: separates a kernel fault from a host-stage fault."""
    from wu import _lib, jpeg
    cases = [(f"440_{s}", P.make_440(s, seed=s)) for s in (1, 2, 7, 16, 17, 33, 97)] + [("420", R.encode(R.synth(33, 17, 1), dict(quality=75)))]
    lib = _lib.load()
    dec = [jpeg.entropy_decode(d, coverage="extended") for _, d in cases]
    assert [d[2].mode for d in dec] == [jpeg.MODE_H1V2] * 7 + [jpeg.MODE_H2V2]
    n = len(cases)
    desc = np.zeros((n, 16), dtype=np.int32)
    qtab = np.zeros((n, 3, 64), dtype=np.uint16)
    tiles, coefs = [], []
    for i, (planes, q, info) in enumerate(dec):
        first_tile = len(tiles)
        nt = -(-info.total_blocks // 32)
        flat = np.zeros(nt * 32 * 64, dtype=np.int16)
        flat[:info.total_blocks * 64] = np.concatenate([p.reshape(-1) for p in planes])
        coefs.append(flat)
        tiles += [i] * nt
        desc[i, :10] = (first_tile * 32, info.height, info.width, info.mode, info.blocks_w[0], info.blocks_h[0], info.blocks_w[1], info.blocks_h[1],
                        first_tile, info.total_blocks)
        qtab[i] = q
    hmax, wmax = max(d[2].height for d in dec), max(d[2].width for d in dec)
    coef_d = torch.from_numpy(np.concatenate(coefs)).to(DEV)
    desc_d, qtab_d = torch.from_numpy(desc).to(DEV), torch.from_numpy(qtab.view(np.int16)).to(DEV)
    tile_d = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.wu_jpeg_workspace_bytes(len(tiles) * 32), dtype=torch.uint8, device=DEV)
    out = torch.full((n, hmax, wmax, 3), 77, dtype=torch.uint8, device=DEV)
    _lib.call("wu_jpeg_reconstruct", coef_d.data_ptr(), desc_d.data_ptr(), tile_d.data_ptr(), qtab_d.data_ptr(), ws.data_ptr(), ws.numel(),
              out.data_ptr(), n, hmax, wmax, len(tiles), torch.cuda.current_stream().cuda_stream)
    _check(out, [(d[2].height, d[2].width) for d in dec], [c for _, c in cases], [nm for nm, _ in cases], want=[P.reconstruct(d) for d in dec])


def test_fid_statistics_with_extended_decode_are_identical(tmp_path):
    """`python -m wu.fid --gpu-decode-extended` over progressive files: the same uint8 batches as the Pillow read path, hence identical
    statistics -- and the files were decoded natively."""
    import _inception_ref as IRF
    from PIL import Image
    from wu import files
    from wu.fid import statistics_of_path
    from wu.inception import InceptionV3
    d = tmp_path / "imgs"
    d.mkdir()
    for k in range(10):
        Image.fromarray(R.synth(96, 128, 40 + k)).save(d / f"img_{k:02d}.jpg", quality=90 if k % 2 else 75, subsampling=k % 3, progressive=True)
    model = InceptionV3([0])
    model.load_state_dict(IRF.make_params(True, seed=6))
    mu0, sig0 = statistics_of_path(str(d), model, 5)
    mu1, sig1 = statistics_of_path(str(d), model, 5, gpu_extended=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sig0, sig1)
    with files.pass_decoder(gpu_extended=True) as dec:
        for _ in files.read_batches(files.image_files(str(d)), 5, dec):
            pass
        assert dec.stats == {"native": 10, "fallback": 0, "fallback_reasons": {}}
