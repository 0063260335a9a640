"""CPU: the JPEG encoder's specification and its host half.  tests/_jpeg_enc_ref.py restates libjpeg's default compress path in
numpy; here it is held against live Pillow and against the stored fixtures (so the GPU test's reference is itself pinned), the
library's header against Pillow's for every quality, and the ABI's size functions and argument checks, all without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import _jpeg_enc_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc")
HEADER_BYTES = 623


def _fixtures():
    stems = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npy"))
    out = []
    for s in stems:
        size, content, q, sub = s.split("_")
        with open(os.path.join(GOLDEN, s + ".jpg"), "rb") as fh:
            out.append((s, np.load(os.path.join(GOLDEN, s + ".npy")), int(q[1:]), {"420": "4:2:0", "444": "4:4:4"}[sub], fh.read()))
    return out


@pytest.mark.parametrize("quality", R.QUALITIES, ids=lambda q: f"q{q}")
def test_restatement_equals_live_pillow_on_the_grid(quality):
    """The 156-case grid (13 sizes x 4 contents x 3 qualities) at Pillow's default subsampling."""
    n = 0
    for h, w in R.SIZES:
        for content in R.CONTENTS:
            img = R.make_image(h, w, content)
            assert R.encode(img, quality) == R.pillow_jpeg(img, quality), (h, w, content, quality)
            n += 1
    assert n == 52


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
def test_restatement_equals_live_pillow_on_the_extra_sizes_and_444(subsampling):
    """12x12, 50x16 (even h, no multiple of 16: the downsampled-row rule), 4x4; and subsampling=0 over every size."""
    sizes = R.EXTRA_SIZES if subsampling == "4:2:0" else R.SIZES + R.EXTRA_SIZES
    for h, w in sizes:
        for content in R.CONTENTS:
            for quality in R.QUALITIES:
                img = R.make_image(h, w, content)
                want = R.pillow_jpeg(img, quality, 0 if subsampling == "4:4:4" else None)
                assert R.encode(img, quality, subsampling) == want, (h, w, content, quality, subsampling)


def test_grid_reaches_the_hard_symbols():
    """The cases are only worth their time if they contain what can go wrong: ZRL runs, blocks without EOB, DC category 11, dummy
    blocks, stuffed 0xFF bytes."""
    seen = {"zrl": False, "no_eob": False, "dc11": False, "stuffing": False, "dummy": False}
    for h, w in R.GPU_SIZES:
        for content in R.CONTENTS:
            for quality in R.QUALITIES:
                st = R.stages(R.make_image(h, w, content), quality)
                blocks, comp = st["blocks"], st["comp"]
                seen["no_eob"] |= bool((blocks[:, 63] != 0).any())
                seen["stuffing"] |= st["raw"].count(b"\xff") >= 4
                seen["dummy"] |= len(blocks) > 0 and (-(-h // 8) % 2 == 1 or -(-w // 8) % 2 == 1)
                for c in range(3):
                    dc = blocks[comp == c][:, 0]
                    seen["dc11"] |= bool((np.abs(np.diff(np.concatenate([[0], dc]))) >= 1024).any())
                nz = blocks[:, 1:] != 0
                for row in nz:
                    idx = np.flatnonzero(row)
                    seen["zrl"] |= bool(len(idx) and (np.diff(np.concatenate([[-1], idx])) > 16).any())
    assert all(seen.values()), seen


def test_restatement_equals_the_fixtures():
    fx = _fixtures()
    assert len(fx) == 12
    for name, img, quality, sub, want in fx:
        assert R.encode(img, quality, sub) == want, name


def test_fixtures_equal_live_pillow():
    """A different Pillow / libjpeg on this machine shows HERE, not as an encoder fault."""
    for name, img, quality, sub, want in _fixtures():
        assert R.pillow_jpeg(img, quality, 0 if sub == "4:4:4" else 2) == want, name


def test_header_equals_pillows_for_every_quality():
    from wu import jpeg_enc
    img = R.make_image(24, 40, "gradient")
    for sub, ps in (("4:2:0", 2), ("4:4:4", 0)):
        for q in range(1, 101):
            want = R.pillow_jpeg(img, q, ps)[:HEADER_BYTES]
            got = jpeg_enc.header(24, 40, q, sub)
            assert len(got) == HEADER_BYTES and got == want, (q, sub)
            assert got == R.header(24, 40, q, sub)
    assert jpeg_enc.header(65535, 1, 75, "4:2:0") == R.header(65535, 1, 75, "4:2:0")
    assert jpeg_enc.header(300, 513) == R.pillow_jpeg(np.zeros((300, 513, 3), np.uint8))[:HEADER_BYTES]        # Pillow's defaults
    ql, qc = R.quant_tables(37)
    assert np.array_equal(jpeg_enc.quant_tables(37), np.stack([ql, qc]))


def test_abi_sizes_and_argument_errors_without_a_gpu():
    from wu import _lib, jpeg_enc
    lib = _lib.load()
    assert lib.wu_jpeg_enc_header_bytes() == HEADER_BYTES and lib.wu_jpeg_enc_desc_bytes() == 16
    # workspace: grows with every argument, 0 for what cannot be encoded
    base = lib.wu_jpeg_enc_workspace_bytes(4, 64, 64, 0, 64 * 64 * 3)
    assert base > 4 * (24 * 128 + 64 * 64 * 3)                      # 24 blocks of 64 int16 and the raw slot per image, at least
    assert lib.wu_jpeg_enc_workspace_bytes(8, 64, 64, 0, 64 * 64 * 3) > base
    assert lib.wu_jpeg_enc_workspace_bytes(4, 65, 64, 0, 64 * 64 * 3) > base
    assert lib.wu_jpeg_enc_workspace_bytes(4, 64, 64, 1, 64 * 64 * 3) > base          # 4:4:4: 3 blocks per 8 x 8 instead of 6 per 16 x 16
    for bad in ((0, 64, 64, 0, 100), (4, 0, 64, 0, 100), (4, 64, 70000, 0, 100), (4, 64, 64, 2, 100), (4, 64, 64, 0, 0), (4, 64, 64, 0, 1 << 28)):
        assert lib.wu_jpeg_enc_workspace_bytes(*bad) == 0, bad
    assert lib.wu_jpeg_enc_out_stride(1000) >= HEADER_BYTES + 1000 + 2 and lib.wu_jpeg_enc_out_stride(1000) % 256 == 0
    assert lib.wu_jpeg_enc_out_stride(0) == 0
    lay = (ctypes.c_longlong * 8)()
    assert lib.wu_jpeg_enc_workspace_layout(2, 33, 17, 0, 4096, lay) == 0
    assert lay[6] == 2 * 3 * 6 and lay[7] == 4096 and list(lay[:6]) == sorted(lay[:6]) and lay[0] == 0       # 2 x 3 MCUs of 6 blocks
    assert lib.wu_jpeg_enc_workspace_layout(2, 33, 17, 5, 4096, lay) < 0 and b"subsampling" in lib.wu_last_error()
    # header
    buf = (ctypes.c_uint8 * 700)()
    assert lib.wu_jpeg_enc_header(8, 8, 75, 0, buf, 700) == HEADER_BYTES
    assert lib.wu_jpeg_enc_header(8, 8, 0, 0, buf, 700) < 0 and b"quality" in lib.wu_last_error()
    assert lib.wu_jpeg_enc_header(8, 8, 101, 0, buf, 700) < 0
    assert lib.wu_jpeg_enc_header(0, 8, 75, 0, buf, 700) < 0 and b"size" in lib.wu_last_error()
    assert lib.wu_jpeg_enc_header(8, 65536, 75, 0, buf, 700) < 0
    assert lib.wu_jpeg_enc_header(8, 8, 75, 3, buf, 700) < 0 and b"subsampling" in lib.wu_last_error()
    assert lib.wu_jpeg_enc_header(8, 8, 75, 0, buf, 100) < 0 and b"buffer" in lib.wu_last_error()
    assert lib.wu_jpeg_enc_header(8, 8, 75, 0, None, 700) < 0
    assert lib.wu_jpeg_enc_qtables(0, buf) < 0 and lib.wu_jpeg_enc_qtables(50, None) < 0
    # the batch entry point validates before it launches anything
    one = ctypes.c_void_p(256)           # a non-null, aligned pointer that is never dereferenced: every call below fails validation first
    args = dict(src=one, dtype=2, sn=192, sc=1, sy=24, sx=3, desc=one, qtab=one, hdr=one, hdr_stride=624, ws=one, ws_bytes=1 << 30, out=one,
                out_bytes=1 << 30, result=one, N=1, H=8, W=8, sub=0, cap=1024, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.wu_jpeg_enc_encode(*a.values())
    assert call(src=None) < 0 and b"null" in lib.wu_last_error()
    assert call(dtype=7) < 0 and b"dtype" in lib.wu_last_error()
    assert call(N=0) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(sub=2) < 0
    assert call(cap=0) < 0
    assert call(hdr_stride=100) < 0 and b"header stride" in lib.wu_last_error()
    assert call(ws_bytes=16) < 0 and b"workspace too small" in lib.wu_last_error()
    assert call(out_bytes=16) < 0 and b"output too small" in lib.wu_last_error()
    assert call(ws=ctypes.c_void_p(257)) < 0 and b"aligned" in lib.wu_last_error()
    assert call(dtype=0, src=ctypes.c_void_p(258)) < 0 and b"element size" in lib.wu_last_error()
    with pytest.raises(ValueError):
        jpeg_enc.header(8, 8, 75, "4:2:2")
    with pytest.raises(ValueError):
        jpeg_enc.header(8, 8, 0)


def test_encoder_refuses_cpu_tensors_and_bad_batches():
    import torch
    from wu.jpeg_enc import GPUJpegEncoder
    enc = GPUJpegEncoder(device="cuda")                  # constructing needs no GPU
    assert enc.header(16, 16) == R.header(16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.launch(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_batch(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        enc.launch(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        enc.launch(torch.zeros(1, 3, 8, 8, dtype=torch.float16))
    with pytest.raises(ValueError):
        GPUJpegEncoder(quality=0)
    with pytest.raises(ValueError):
        GPUJpegEncoder(subsampling="4:2:2")
    enc.close()
