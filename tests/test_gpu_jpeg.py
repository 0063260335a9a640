"""GPU: the JPEG decoder (wu/jpeg.py, csrc/jpeg.hip) and the batch loader (wu/data.py) against Pillow -- what the reference's
loaders run (dataset.py:64-67: Image.open(path).convert('RGB')).  Bar: exact equality of every byte, inside each image's H x W with
Pillow's decode and zero outside it."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


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


def _mixed():
    """All sizes and modes in ONE batch: offsets, padding and per-image modes together."""
    cases = R.grid(R.SMALL_SIZES) + R.grid(R.LARGE_SIZES, [v for v in R.VARIANTS if v[0] in ("q85_420", "q95_422", "q100_444", "q30_rst3", "q75_rstrow", "grey")])
    for name in ("restart_blocks.jpg", "restart_rows.jpg", "restart_grey.jpg"):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            cases.append((name, fh.read()))
    return cases


def test_decode_batch_mixed_equals_pillow():
    from wu.jpeg import GPUJpegDecoder
    cases = _mixed()
    assert len(cases) >= 150
    dec = GPUJpegDecoder(DEV)
    src, sizes = dec.decode_batch([d for _, d in cases])
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    _check(src, sizes, [d for _, d in cases], [n for n, _ in cases])
    assert dec.stats["fallback"] == 0 and dec.stats["native"] == len(cases)
    with pytest.raises(ValueError):
        dec.decode_batch([])
    dec.close()


def test_device_kernels_alone_equal_the_numpy_restatement():
    """wu_jpeg_reconstruct on coefficients uploaded by the test itself, against _jpeg_ref on the SAME coefficients: separates a kernel
    fault from a Huffman fault."""
    from wu import _lib, jpeg
    cases = R.grid([(97, 131), (33, 17), (120, 161), (224, 224)])
    lib = _lib.load()
    dec = [jpeg.entropy_decode(d) for _, d in cases]
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
        bwc, bhc = (info.blocks_w[1], info.blocks_h[1]) if info.ncomp == 3 else (0, 0)
        desc[i, :10] = (first_tile * 32, info.height, info.width, info.mode, info.blocks_w[0], info.blocks_h[0], bwc, bhc, first_tile, info.total_blocks)
        qtab[i] = q
    hmax, wmax = max(d[2].height for d in dec), max(d[2].width for d in dec)
    coef_d = torch.from_numpy(np.concatenate(coefs)).to(DEV)
    desc_d, qtab_d = torch.from_numpy(desc).to(DEV), torch.from_numpy(qtab.view(np.int16)).to(DEV)
    tile_d = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.wu_jpeg_workspace_bytes(len(tiles) * 32), dtype=torch.uint8, device=DEV)
    out = torch.full((n, hmax, wmax, 3), 77, dtype=torch.uint8, device=DEV)
    _lib.call("wu_jpeg_reconstruct", coef_d.data_ptr(), desc_d.data_ptr(), tile_d.data_ptr(), qtab_d.data_ptr(), ws.data_ptr(), ws.numel(),
              out.data_ptr(), n, hmax, wmax, len(tiles), torch.cuda.current_stream().cuda_stream)
    _check(out, [(d[2].height, d[2].width) for d in dec], [c for _, c in cases], [nm for nm, _ in cases], want=[R.reconstruct(d) for d in dec])
    assert lib.wu_jpeg_reconstruct(coef_d.data_ptr(), desc_d.data_ptr(), tile_d.data_ptr(), qtab_d.data_ptr(), ws.data_ptr(), ws.numel() - 64,
                                   out.data_ptr(), n, hmax, wmax, len(tiles), None) < 0          # validated on the host, nothing launched
    assert b"workspace" in lib.wu_last_error()


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (8, 8), (3, 40), (40, 3), (17, 33), (5, 3), (9, 4), (2, 2), (16, 16), (8, 16), (16, 8), (33, 1)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_sizes_one_image_per_batch(size):
    """N = 1; widths with a down-sampled chroma width <= 2 (replication instead of the fancy filters); exactly one MCU (8x8 4:4:4 and
    grey, 8x16 4:2:2, 16x16 4:2:0)."""
    from wu.jpeg import GPUJpegDecoder
    dec = GPUJpegDecoder(DEV, threads=2)
    for name, data in R.grid([size]):
        src, sizes = dec.decode_batch([data])
        assert tuple(src.shape) == (1, size[0], size[1], 3)
        _check(src, sizes, [data], [name])
    assert dec.stats["fallback"] == 0
    dec.close()


def test_fallback_slots_and_unreadable_file(tmp_path):
    from wu.jpeg import GPUJpegDecoder
    native = R.grid([(64, 48), (97, 131)], R.VARIANTS[:3])
    paths = []
    for name, data in native:
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
    fixtures = ["progressive.jpg", "cmyk.jpg", "rgb.png", "grey.png", "s440.jpg"]
    items = paths[:3] + [os.path.join(GOLDEN, f) for f in fixtures[:2]] + paths[3:] + [os.path.join(GOLDEN, f) for f in fixtures[2:]]
    datas = [open(p, "rb").read() for p in items]
    dec = GPUJpegDecoder(DEV)
    src, sizes = dec.decode_batch(items)
    _check(src, sizes, datas, items)
    with np.load(os.path.join(GOLDEN, "expected.npz")) as exp:                # and the arrays Pillow decoded where the fixtures were written
        for f in fixtures:
            i = items.index(os.path.join(GOLDEN, f))
            h, w = exp[f].shape[:2]
            assert np.array_equal(src[i, :h, :w].cpu().numpy(), exp[f]), f
    assert dec.stats == {"native": 6, "fallback": 5, "fallback_reasons": {"progressive": 1, "colorspace": 1, "not-jpeg": 2, "sampling": 1}}
    src, sizes = dec.decode_batch([os.path.join(GOLDEN, "rgb.png")])          # a batch with no native image at all
    _check(src, sizes, [open(os.path.join(GOLDEN, "rgb.png"), "rb").read()])
    with pytest.raises(RuntimeError, match="truncated.jpg"):
        dec.decode_batch(paths[:2] + [os.path.join(GOLDEN, "truncated.jpg")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GPUJpegDecoder("cpu").decode_batch(paths[:1])
    dec.close()


def test_loader_with_pipeline_equals_the_reference_loader_output(tmp_path):
    """files -> JpegBatchLoader -> GPUInputPipeline(224, augmentation=True) == oracle.input_ref.train_transform on the Pillow-decoded
    arrays with the same draws, bit for bit."""
    from oracle import input_ref as IR
    from wu.data import JpegBatchLoader
    from wu.input_pipeline import GPUInputPipeline
    sizes = [(375, 500), (500, 333), (224, 224), (97, 131), (600, 800), (64, 48), (120, 161)]
    variants = [R.VARIANTS[9], R.VARIANTS[8], R.VARIANTS[12], R.VARIANTS[0], R.VARIANTS[4], R.VARIANTS[7], R.VARIANTS[5]]
    paths, datas = [], []
    for k, ((h, w), (vn, kw)) in enumerate(zip(sizes, variants)):
        data = R.encode(R.synth(h, w, 20 + k), kw)
        p = tmp_path / f"{k}_{vn}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
        datas.append(data)
    labels = np.arange(len(paths)) % 3
    pipe, twin = GPUInputPipeline(224, augmentation=True, seed=13), GPUInputPipeline(224, augmentation=True, seed=13)
    loader = JpegBatchLoader(paths, labels, batch_size=3, pipeline=pipe, shuffle=True, seed=5)
    seen = 0
    for epoch in range(2):
        order = loader.epoch_indices(epoch)
        for images, targets, batch_paths in loader:
            idx = order[seen % len(paths):seen % len(paths) + len(batch_paths)]
            assert batch_paths == [paths[i] for i in idx] and targets.tolist() == [int(labels[i]) for i in idx] and targets.is_cuda
            decoded = [R.pillow_rgb(datas[i]) for i in idx]
            params = twin.draw([a.shape[:2] for a in decoded])                # the same seeded draws, in the same order
            assert tuple(images.shape) == (len(idx), 3, 224, 224) and images.dtype == torch.float32
            for j, (a, p) in enumerate(zip(decoded, params)):
                ref = IR.train_transform(a, 224, p["angle"], p["flip"], True, p["crop"], p["factors"], p["order"])
                assert np.array_equal(images[j].cpu().numpy(), ref), f"epoch {epoch} {batch_paths[j]}"
            seen += len(idx)
    assert seen == 2 * len(paths) and loader.decoder.stats["fallback"] == 0
    loader.close()


def test_replay_and_staging_reuse():
    """The same HostBatch finished twice; then two loaders' batches in flight with prefetch=2 over 20 batches of different content,
    every batch verified: a staging buffer refilled before its copy completed would show here."""
    from wu.data import JpegBatchLoader
    from wu.jpeg import GPUJpegDecoder
    dec = GPUJpegDecoder(DEV)
    cases = R.grid([(120, 161), (64, 48)])
    datas = [d for _, d in cases]
    hb = dec.prepare(datas)
    a, sa = dec.finish(hb)
    b, sb = dec.finish(hb)
    assert sa == sb and torch.equal(a, b)
    _check(b, sb, datas)
    hb.release()
    with pytest.raises(RuntimeError, match="released"):
        dec.finish(hb)
    # 2 x 20 batches of 8, every image different; both loaders share ONE decoder (and so its staging buffers)
    rng_sizes = [(40 + 8 * (k % 7), 56 + 5 * (k % 11)) for k in range(160)]
    files = [R.encode(R.synth(h, w, 100 + k), R.VARIANTS[k % len(R.VARIANTS)][1]) for k, (h, w) in enumerate(rng_sizes)]
    want = {k: R.pillow_rgb(f) for k, f in enumerate(files)}
    l1 = JpegBatchLoader(files, list(range(160)), batch_size=8, decoder=dec, shuffle=True, seed=1, prefetch=2)
    l2 = JpegBatchLoader(files, list(range(160)), batch_size=8, decoder=dec, shuffle=True, seed=2, prefetch=2)
    held, batches = [], 0
    for (x1, t1, _), (x2, t2, _) in zip(l1, l2):
        held.append((x1, t1.tolist()))                                        # verified LATER: after more batches went through the buffers
        held.append((x2, t2.tolist()))
        batches += 1
    assert batches == 20
    for (src, sizes), ids in held:
        _check(src, sizes, [files[k] for k in ids], ids, want=[want[k] for k in ids])
    assert len(dec._staging) <= dec.max_staging
    dec.close()


def test_reconstruct_inside_a_captured_graph():
    from wu.jpeg import GPUJpegDecoder
    dec = GPUJpegDecoder(DEV)
    cases = R.grid([(97, 131), (40, 3), (64, 48)])
    datas = [d for _, d in cases]
    hb = dec.prepare(datas)
    db = dec.upload(hb)
    eager = dec.reconstruct(db)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dec.reconstruct(db, out)
    for _ in range(3):
        out.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    _check(out, hb.sizes, datas)
    # new coefficients in the same device buffers: the replay decodes them (same shapes: the same files in another order)
    perm = [datas[(i + len(R.VARIANTS)) % len(datas)] for i in range(len(datas))]
    hb2 = dec.prepare(perm)
    assert hb2.used == hb.used and hb2.n_tiles == hb.n_tiles and (hb2.hmax, hb2.wmax) == (hb.hmax, hb.wmax)
    db.buf.copy_(hb2.staging.tensor[:hb2.used], non_blocking=True)
    g.replay()
    torch.cuda.synchronize()
    _check(out, hb2.sizes, perm)
    dec.close()


def test_fid_statistics_with_gpu_decode_are_identical(tmp_path):
    """`python -m wu.fid --gpu-decode`: the same bytes in, the same uint8 batches out, hence identical statistics."""
    import _inception_ref as IRF
    from PIL import Image
    from wu.fid import statistics_of_path
    from wu.inception import InceptionV3
    d = tmp_path / "imgs"
    d.mkdir()
    for k in range(12):
        Image.fromarray(R.synth(96, 128, 40 + k)).save(d / f"img_{k:02d}.jpg", quality=90 if k % 2 else 75, subsampling=k % 3)
    Image.fromarray(R.synth(96, 128, 60)).save(d / "img_12.png")
    model = InceptionV3([0])
    model.load_state_dict(IRF.make_params(True, seed=6))
    mu0, sig0 = statistics_of_path(str(d), model, 5)
    mu1, sig1 = statistics_of_path(str(d), model, 5, gpu_decode=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sig0, sig1)
