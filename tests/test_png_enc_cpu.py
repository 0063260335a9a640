"""CPU: the PNG encoder's specification and its host half.  tests/_png_enc_ref.py restates csrc/png_enc.hip; here that restatement is
itself held against what it must satisfy whatever the kernels do -- Pillow decodes its files to the input pixels with every CRC right,
zlib inflates them with the Adler-32 right, the row filters are the minimum-sum-of-absolute-differences choice, no file exceeds the
stored-block bound, and literal-only Huffman coding costs what zlib's own Huffman-only mode costs."""
import ctypes
import io
import zlib

import numpy as np
import pytest

import _png_enc_ref as R

# File size over zlib's Z_HUFFMAN_ONLY stream (level 6, memLevel 9) of the same filtered bytes in the same framing, measured per
# compressible case (profiles/png_enc_bench.md): between 0.9932 and 1.00024.  The bar is the worst measured ratio plus 2 % for the
# per-segment table overhead of inputs that are not in the grid; a code-length construction that needed 1.10 would be wrong.
WORST_MEASURED_RATIO = 1.00025
RATIO_BOUND = WORST_MEASURED_RATIO + 0.02

_cache = {}


def _case(case):
    if case not in _cache:
        img = R.make_image(*case)
        _cache[case] = (img, R.stages(img))
    return _cache[case]


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_restatement_decodes_in_pillow_to_the_input(case):
    from PIL import Image
    img, st = _case(case)
    Image.open(io.BytesIO(st["file"])).verify()               # every chunk's CRC
    im = Image.open(io.BytesIO(st["file"]))
    assert im.mode == "RGB" and im.size == (case[1], case[0])
    assert np.array_equal(np.asarray(im), img)


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_chunks_checksums_and_filter_choice(case):
    h, w, _ = case
    img, st = _case(case)
    chunks = R.parse_chunks(st["file"])                       # asserts zlib.crc32 of every chunk
    kinds = [k for k, _ in chunks]
    nseg = -(-h * (1 + 3 * w) // R.SEGMENT)
    assert kinds == [b"IHDR"] + [b"IDAT"] * nseg + [b"IEND"]
    z = b"".join(b for k, b in chunks if k == b"IDAT")
    raw = zlib.decompress(z)                                  # checks the Adler-32
    assert len(raw) == h * (1 + 3 * w) and raw == st["filtered"]
    assert R.unpack(st["file"])[:2] == (h, w)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert np.array_equal(rows[:, 0], R.filter_types_vectorised(img))


def test_grid_reaches_every_mechanism():
    """The cases are only worth their names if they reach what they are named for."""
    types = set()
    for case in R.GRID:
        types |= set(R.filter_types_vectorised(R.make_image(*case)).tolist())
    assert types == {0, 1, 2, 3, 4}
    assert _case((64, 64, "noise"))[1]["stored"] == [True] and _case((1, 1, "noise"))[1]["stored"] == [True]
    assert len(_case((200, 300, "natural"))[1]["segments"]) == 6 and 200 * 901 % R.SEGMENT != 0
    assert len(_case((128, 85, "gradient_noise"))[1]["filtered"]) == R.SEGMENT
    assert len(_case((99, 110, "gradient_noise"))[1]["filtered"]) == R.SEGMENT + 1
    assert len(_case((99, 110, "gradient_noise"))[1]["segments"]) == 2
    flat = _case((16, 16, "flat"))[1]
    assert flat["stored"] == [False] and len(set(flat["filtered"])) <= 6         # almost one symbol: zeros, with the filter bytes and one pixel


def test_code_lengths_are_complete_limited_and_handle_few_symbols():
    rng = np.random.default_rng(0)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for freq, maxbits in ((fib, 15), (fib[:19], 7), ([0, 5, 0, 0, 1], 15), ([3, 3], 7), ([1] * 257, 15),
                          (rng.integers(0, 50, 257).tolist(), 15), (rng.integers(0, 3, 19).tolist(), 7), ((rng.integers(1, 4000, 257) ** 2).tolist(), 15)):
        lens = R.code_lengths(freq, maxbits)
        used = [l for l in lens if l]
        assert all((l > 0) == (f > 0) for l, f in zip(lens, freq)) and max(used) <= maxbits
        assert sum(2.0 ** -l for l in used) == 1.0, (freq, lens)              # complete: inflate refuses anything else
        order = sorted(range(len(freq)), key=lambda s: freq[s])
        assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]) if freq[a] and freq[a] < freq[b])       # rarer is never shorter
        codes = R.canonical_codes(lens)
        assert len({(c, l) for c, l in zip(codes, lens) if l}) == len(used)
    assert R.code_lengths([0, 0, 7, 0], 15) == [0, 0, 1, 0]                     # one symbol: one bit (never reached by the encoder)
    assert max(R.code_lengths(fib, 15)) == 15 and len(fib) == 30                # Huffman's own depth would be 29: the limit did bite
    # the run-length tokens expand to the sequence
    for seq in ([0] * 258, [8] * 258, [0] * 10 + [3] * 7 + [0] * 139 + [5, 5, 0, 0, 1], rng.integers(0, 3, 258).tolist()):
        out = []
        for s, e in R.length_tokens(seq):
            out += [0] * (e + 11) if s == 18 else [0] * (e + 3) if s == 17 else [out[-1]] * (e + 3) if s == 16 else [s]
        assert out == seq


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_size_is_bounded_by_stored_blocks(case):
    h, w, _ = case
    _, st = _case(case)
    assert len(st["file"]) <= R.out_stride(h, w)
    for seg, stored, at in zip(st["segments"], st["stored"], range(0, len(st["filtered"]), R.SEGMENT)):
        n = min(R.SEGMENT, len(st["filtered"]) - at)
        assert len(seg) == n + 5 if stored else len(seg) < n + 5


@pytest.mark.parametrize("case", R.COMPRESSIBLE, ids=R.case_id)
def test_size_against_zlib_huffman_only(case):
    h, w, _ = case
    _, st = _case(case)
    ratio = len(st["file"]) / R.huffman_only_file(h, w, st["filtered"])
    print(f"{R.case_id(case)}: {len(st['file'])} bytes, {ratio:.4f} x zlib Z_HUFFMAN_ONLY")
    assert ratio <= RATIO_BOUND


def test_abi_agrees_with_the_restatement_without_a_gpu():
    from wu import _lib, png_enc
    lib = _lib.load()
    assert lib.wu_png_enc_desc_bytes() == 16
    assert lib.wu_png_enc_segment_bytes() == R.SEGMENT == png_enc.segment_bytes()
    for h, w in [(c[0], c[1]) for c in R.GRID] + [(224, 224), (512, 512), (1, 10922), (10922, 1), (4096, 4096)]:
        assert lib.wu_png_enc_out_stride(h, w) == R.out_stride(h, w) == png_enc.out_stride(h, w), (h, w)
    base = lib.wu_png_enc_workspace_bytes(4, 64, 64)
    assert base >= 4 * (64 * 193 + 64 * 193 + 5)              # the filtered stream and one slot per image, at least
    assert lib.wu_png_enc_workspace_bytes(8, 64, 64) > base and lib.wu_png_enc_workspace_bytes(4, 200, 64) > base
    for bad in ((0, 64, 64), (4, 0, 64), (4, 64, 0), (4, 64, 70000), (4, 70000, 64), (1, 65535, 65535)):
        assert lib.wu_png_enc_workspace_bytes(*bad) == 0, bad
    assert lib.wu_png_enc_out_stride(0, 8) == 0
    with pytest.raises(ValueError):
        png_enc.out_stride(0, 8)
    # the batch entry point validates before it launches anything
    one = ctypes.c_void_p(256)           # a non-null, aligned pointer that is never dereferenced: every call below fails validation first
    args = dict(src=one, dtype=2, sn=192, sc=1, sy=24, sx=3, desc=one, ws=one, ws_bytes=1 << 30, out=one, out_bytes=1 << 30, result=one,
                N=1, H=8, W=8, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.wu_png_enc_encode(*a.values())
    assert call(src=None) < 0 and b"null" in lib.wu_last_error()
    assert call(dtype=7) < 0 and b"dtype" in lib.wu_last_error()
    assert call(N=0) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(W=70000) < 0 and b"bad shape" in lib.wu_last_error()
    assert call(sy=-24) < 0 and b"negative" in lib.wu_last_error()
    assert call(ws_bytes=16) < 0 and b"workspace too small" in lib.wu_last_error()
    assert call(out_bytes=16) < 0 and b"output too small" in lib.wu_last_error()
    assert call(ws=ctypes.c_void_p(257)) < 0 and b"aligned" in lib.wu_last_error()
    assert call(dtype=0, src=ctypes.c_void_p(258)) < 0 and b"element size" in lib.wu_last_error()


def test_encoder_refuses_cpu_tensors_and_bad_batches():
    import torch
    from wu.png_enc import GPUPngEncoder
    enc = GPUPngEncoder(device="cuda")                   # constructing needs no GPU
    assert enc.segment_bytes == R.SEGMENT and enc.stats == {"native": 0, "bytes": 0}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.launch(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_batch(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        enc.launch(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        enc.launch(torch.zeros(1, 3, 8, 8, dtype=torch.float16))
    with pytest.raises(ValueError):
        enc.save_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), ["a.png"])
    enc.close()


def test_drivers_keep_png_on_pillow_without_an_encoder(tmp_path):
    """png_encoder=None changes nothing: the signature defaults, and a CPU batch still goes through Pillow."""
    import inspect
    import torch
    from PIL import Image
    from wu import infer_driver as D
    assert inspect.signature(D.save_images).parameters["png_encoder"].default is None
    assert inspect.signature(D.class_sweep_to_dir).parameters["png_encoder"].default is None
    x = torch.rand(2, 3, 9, 7, generator=torch.Generator().manual_seed(0))
    paths = [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    D.save_images(x, paths, normalize=False)
    want = D.to_uint8(x).numpy()
    for p, rgb in zip(paths, want):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "PNG")
        with open(p, "rb") as fh:
            assert fh.read() == buf.getvalue()
