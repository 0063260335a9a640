"""The colour-transfer baseline on the GPU (csrc/colour_ot.hip through the C ABI, wu.colour) against tests/_colour_ref.py.

Everything is compared with np.array_equal: both sides do the same float64 operations in the same order without FMA, sorting is exact, and
the mid-rank rule leaves nothing to a tie-break -- there is no tolerance anywhere.  Shapes bracket the sort's block (b = wu_swd_sort_block():
1 x (b - 1), 1 x b, 1 x (b + 1), where the LDS sample of a sorted column changes its stride too), the ragged 48 x 40, 64 x 128 with several
workgroups per image, and the degenerate 1 x 1 and 1 x 7; P covers 1, 2, n, n - 1, 3 n + 1 and a P beyond one sort block.

ABI-level outputs live in tests/_gpu_guard.py buffers: NaN before the call, guards on both sides checked after it; workspaces start as 0xFF."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _colour_cases as CASES
import _colour_ref as R
from _gpu_guard import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}
NAMES = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.uint8: "uint8"}


def _lib():
    from wu import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _block():
    return _lib()[1].wu_swd_sort_block()


class GuardedF64(Guarded):
    """n doubles inside a Guarded float buffer: two NaN floats side by side are a NaN double, and the payload starts 128 bytes in."""

    def __init__(self, n, init=None):
        super().__init__(2 * n)
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64).reshape(-1).view(np.float32)))

    def numpy(self, what, shape=None):
        out = super().numpy(what).view(np.float64)
        return out.reshape(shape) if shape is not None else out


def _rot(R9):
    return (ctypes.c_double * 9)(*np.asarray(R9, dtype=np.float64).reshape(-1).tolist())


def _mapping(value_range):
    from wu import paired
    return paired.range_mapping(value_range)


def _host(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _abi_transfer(x, palettes, targets, rots, step, value_range):
    """load -> (palette_keys, step) per rotation -> store, on a float32 NCHW batch, every buffer guarded; returns (R, B, 3, H, W)."""
    L, lib = _lib()
    b, _, h, w = x.shape
    n, (c, p, _) = h * w, palettes.shape
    r = len(targets)
    nimg = r * b
    nbytes = lib.wu_colour_ot_workspace_bytes(nimg, n, c, p)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    pal = torch.from_numpy(np.ascontiguousarray(palettes, dtype=np.float64)).to(DEV)
    cls = torch.tensor([t for t in targets for _ in range(b)], dtype=torch.int32, device=DEV)
    state, keys, out = GuardedF64(nimg * 3 * n), GuardedF64(c * 3 * p), Guarded(nimg * 3 * n)
    scale, shift, rng = _mapping(value_range)
    L.call("wu_colour_ot_load", xd.data_ptr(), *xd.stride(), 0, b, h, w, scale, shift, rng, 0, nimg, state.ptr, _stream())
    for k in range(len(rots)):
        L.call("wu_colour_ot_palette_keys", pal.data_ptr(), c, p, _rot(rots[k]), keys.ptr, ws.data_ptr(), _stream())
        L.call("wu_colour_ot_step", state.ptr, nimg, n, keys.ptr, c, p, cls.data_ptr(), _rot(rots[k]), step, ws.data_ptr(), _stream())
    lo, hi = value_range
    L.call("wu_colour_ot_store", state.ptr, 0, nimg, out.ptr, b * 3 * n, 3 * n, n, w, 1, 0, b, h, w, float(lo), float(hi) - float(lo), 0,
           _stream())
    torch.cuda.synchronize()
    state.numpy("wu_colour_ot_step (state)")
    keys.numpy("wu_colour_ot_palette_keys")
    return out.numpy("wu_colour_ot_store", (r, b, 3, h, w))


def _shape_cases():
    b = 8192                      # wu_swd_sort_block(), asserted in the test: parametrisation happens before a library is loaded
    return [
        # h, w, P, B, targets, K, step
        (1, 1, 1, 1, [0], 1, 1.0),
        (1, 1, 4, 2, [1, 0, 1], 2, 0.5),
        (1, 7, 6, 2, [0], 2, 1.0),
        (1, 7, 22, 1, [0, 1, 2], 5, 0.5),
        (1, b - 1, 2, 1, [0], 2, 1.0),
        (1, b, b, 1, [1], 2, 1.0),
        (1, b + 1, b, 2, [0, 2, 2], 1, 1.0),
        (1, b + 1, b + 5, 1, [0], 2, 0.5),
        (48, 40, 1, 1, [0], 2, 1.0),
        (48, 40, 3 * 48 * 40 + 1, 2, [2, 0, 1], 5, 1.0),
        (64, 128, 64 * 128, 1, [0], 2, 1.0),
        (64, 128, 64 * 128 - 1, 2, [1, 1, 0], 1, 0.5),
        (64, 128, 3 * 64 * 128 + 1, 1, [0], 5, 1.0),
    ]


@pytest.mark.parametrize("h,w,p,b,targets,k,step", _shape_cases())
def test_pipeline_bit_exact_through_the_abi(h, w, p, b, targets, k, step):
    from wu import colour
    assert _block() == 8192
    x = CASES.images(b, h, w, seed=h + w + p)
    pal = CASES.palettes(3, p, seed=p + k)
    rots = colour.draw_rotations(k + 1, k)
    want = R.transfer(x, pal, targets, rots, step, (-1, 1), _mapping((-1, 1)), "float32")
    got = _abi_transfer(x, pal, targets, rots, step, (-1, 1))
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} values differ"
    if h * w > 1 and p > 2:
        assert np.abs(want - x[None]).max() > 0.01                       # the colours moved: not a trivially-equal comparison
    via = colour.transfer(torch.from_numpy(x).to(DEV), torch.from_numpy(pal).to(DEV), targets, k, k + 1, step, (-1, 1))
    assert via.shape == (len(targets), b, 3, h, w) and via.dtype == torch.float32 and via.is_cuda
    assert np.array_equal(via.cpu().numpy(), want)


def _input_kinds(n, h, w, seed):
    """(name, CUDA tensor of some layout, the values the kernel must see as a numpy array, value_range): the four of test_gpu_swd.py."""
    x = CASES.images(n, h, w, seed)
    yield "float32 NCHW", torch.from_numpy(x).to(DEV), x, (-1, 1)
    xb = torch.from_numpy(x).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert n == 1 or xb.stride(1) == 1
    yield "bf16 channels-last", xb, xb.float().cpu().numpy(), (-1, 1)
    u = CASES.images_u8(n, h, w, seed + 1)
    ud = torch.from_numpy(np.ascontiguousarray(u.transpose(0, 2, 3, 1))).to(DEV).permute(0, 3, 1, 2)
    assert ud.stride(1) == 1 and not ud.is_contiguous()
    yield "uint8 NHWC view", ud, u, "uint8"
    big = CASES.images(n, h + 5, w + 7, seed + 2)
    crop = torch.from_numpy(big).to(DEV)[:, :, 2:2 + h, 3:3 + w]
    assert crop.storage_offset() > 0
    yield "cropped view", crop, big[:, :, 2:2 + h, 3:3 + w], (0, 1)


def _check(name, xd, seen, value_range, pal, targets, iters, seed, step, max_images=None):
    from wu import colour
    want = R.transfer(seen, pal, targets, colour.draw_rotations(seed, iters), step, value_range, _mapping(value_range), NAMES[xd.dtype])
    before = xd.clone()
    got = colour.transfer(xd, colour.ClassPalettes(pal), targets, iters, seed, step, value_range, max_images)
    assert got.dtype == xd.dtype and tuple(got.shape) == (len(targets),) + tuple(xd.shape), name
    assert np.array_equal(_host(got), want), f"{name}: {(_host(got) != want).sum()} of {want.size} values differ"
    assert torch.equal(xd, before), f"{name}: input modified"
    return got


@pytest.mark.parametrize("b,h,w,p,targets,k,step", [(2, 48, 40, 777, [1, 0, 1], 2, 1.0), (1, 1, 7, 5, [0, 1], 5, 0.5)])
def test_input_kinds(b, h, w, p, targets, k, step):
    pal = CASES.palettes(2, p, seed=21)
    for name, xd, seen, value_range in _input_kinds(b, h, w, seed=h + w):
        _check(name, xd, seen, value_range, pal, targets, k, 3, step)


def test_uint8_range_on_a_float_tensor_and_float_range_on_bytes():
    pal = CASES.palettes(2, 300, seed=22)
    u = CASES.images_u8(2, 9, 11, 23)
    _check("float bytes", torch.from_numpy(u.astype(np.float32)).to(DEV), u.astype(np.float32), "uint8", pal, [1, 0], 2, 0, 1.0)
    _check("bytes, (0, 255)", torch.from_numpy(u).to(DEV), u, (0, 255), pal, [0], 2, 0, 1.0)


@pytest.mark.parametrize("case", ["flat", "flat across blocks", "two colours", "two colours across blocks", "uint8 noise",
                                  "repeated palette"])
def test_ties(case):
    b1 = _block() + 1
    pal = CASES.palettes(2, 500, seed=31)
    if case == "flat":                       # every pixel: lo = 0, hi = n
        x = CASES.flat(2, 20, 13)
    elif case == "flat across blocks":
        x = CASES.flat(1, 1, b1)
    elif case == "two colours":
        x = CASES.two_colour(2, 20, 13, 32)
    elif case == "two colours across blocks":
        x = CASES.two_colour(1, 1, b1, 33)
    elif case == "uint8 noise":
        u = CASES.noise_u8(2, 48, 40, 34)
        got = _check(case, torch.from_numpy(u).to(DEV), u, "uint8", pal, [0, 1], 3, 1, 1.0)
        assert len(np.unique(got[0, 0].cpu().numpy().reshape(3, -1), axis=1).T) <= len(np.unique(u[0].reshape(3, -1), axis=1).T)
        return
    else:
        x, pal = CASES.images(2, 20, 13, 35), CASES.repeated_palette(2, 64)
    got = _check(case, torch.from_numpy(x).to(DEV), x, (-1, 1), pal, [1, 0], 3, 1, 1.0)
    if case.startswith("flat"):              # a flat image stays flat
        g = got.cpu().numpy()
        assert (g == g[..., :1, :1]).all()


@pytest.mark.parametrize("kind", ["noise", "ties"])
def test_own_pixels_as_palette_return_the_image(kind):
    from wu import colour
    x = CASES.images(1, 48, 40, 41) if kind == "noise" else CASES.two_colour(1, 48, 40, 42)
    pal = R.load_state(x, *_mapping((-1, 1)))[0].T[None]                 # (1, n, 3): P = n, the image's own pixels
    got = colour.transfer(torch.from_numpy(x).to(DEV), pal, [0], iters=5, seed=2)
    assert np.array_equal(got[0].cpu().numpy(), x)
    u = CASES.noise_u8(1, 48, 40, 43)
    pal = R.load_state(u, 1.0, 0.0, 255.0)[0].T[None]
    got = colour.transfer(torch.from_numpy(u).to(DEV), pal, [0], iters=5, seed=2, step=0.5, value_range="uint8")
    assert np.array_equal(got[0].cpu().numpy(), u)


def test_one_iteration_takes_every_channel_to_the_palette_channel():
    from wu import colour
    n = 2048
    x = CASES.distinct_integer_image(n, 51)
    pal = CASES.distinct_integer_image(n, 52).reshape(3, n).T.astype(np.float64)
    got = colour.transfer(torch.from_numpy(x).to(DEV), pal[None], [0], iters=1, value_range=(0, 1))[0, 0].cpu().numpy().reshape(3, n)
    for c in range(3):
        assert np.array_equal(np.sort(got[c]), np.sort(pal[:, c]).astype(np.float32))
        assert np.array_equal(np.argsort(got[c]), np.argsort(x[0, c, 0]))       # the order of the pixels is kept


def test_chunking_and_repeats_give_the_same_bytes():
    from wu import colour
    x = torch.from_numpy(CASES.images(2, 48, 40, 61)).to(DEV).to(torch.bfloat16)
    pal = colour.ClassPalettes(CASES.palettes(3, 1000, seed=62)).to(DEV)
    base = colour.transfer(x, pal, [2, 0, 2], iters=3, seed=5)
    for max_images in (1, 2, 4, 6, 100):
        assert torch.equal(colour.transfer(x, pal, [2, 0, 2], iters=3, seed=5, max_images=max_images), base), max_images
    assert torch.equal(colour.transfer(x, pal, [2, 0, 2], iters=3, seed=5), base)
    assert torch.equal(base[0], base[2]) and not torch.equal(base[0], base[1])   # repeated targets agree, distinct ones do not
    assert not torch.equal(colour.transfer(x, pal, [2, 0, 2], iters=3, seed=6), base)


def test_step_on_a_hand_set_state_under_a_signed_permutation():
    L, lib = _lib()
    n, p, npal = 100, 37, 2
    rot = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    rng = np.random.RandomState(71)
    s0 = np.round(rng.uniform(-0.5, 1.5, (3, 3, n)) * 64) / 64            # outside [0, 1] too, with ties
    pal = CASES.palettes(npal, p, seed=72)
    classes = [1, 0, 7]                                                   # the last one has no palette: its image must stay as it is
    nbytes = lib.wu_colour_ot_workspace_bytes(3, n, npal, p)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    state, keys = GuardedF64(3 * 3 * n, s0), GuardedF64(npal * 3 * p)
    pal_d = torch.from_numpy(pal).to(DEV)
    cls = torch.tensor(classes, dtype=torch.int32, device=DEV)
    L.call("wu_colour_ot_palette_keys", pal_d.data_ptr(), npal, p, _rot(rot), keys.ptr, ws.data_ptr(), _stream())
    L.call("wu_colour_ot_step", state.ptr, 3, n, keys.ptr, npal, p, cls.data_ptr(), _rot(rot), 0.75, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    want_keys = np.stack([np.sort(R.project(rot, np.ascontiguousarray(pal[c].T)), axis=1) for c in range(npal)]).reshape(npal * 3, p)
    assert np.array_equal(keys.numpy("wu_colour_ot_palette_keys", (npal * 3, p)), want_keys)
    got = state.numpy("wu_colour_ot_step", (3, 3, n))
    assert np.array_equal(got[0], R.step(s0[0], pal[1], rot, 0.75))
    assert np.array_equal(got[1], R.step(s0[1], pal[0], rot, 0.75))
    assert np.array_equal(got[2], s0[2])


def test_out_of_range_sizes_are_refused_before_any_launch():
    L, lib = _lib()
    big = (1 << 21) + 1
    state, keys, out = GuardedF64(64), GuardedF64(64), Guarded(64)
    ws = torch.full((4096,), 0xFF, dtype=torch.uint8, device=DEV)
    x = torch.zeros(1, 3, 2, 2, device=DEV)
    cls = torch.zeros(4, dtype=torch.int32, device=DEV)
    rot = _rot(np.eye(3))
    for nimg, n, npal, p in ((0, 4, 1, 4), (1, 0, 1, 4), (1, big, 1, 4), (1, 4, 0, 4), (1, 4, 1, 0), (1, 4, 1, big)):
        assert lib.wu_colour_ot_workspace_bytes(nimg, n, npal, p) == 0
        assert lib.wu_colour_ot_step(state.ptr, nimg, n, keys.ptr, npal, p, cls.data_ptr(), rot, 1.0, ws.data_ptr(), _stream()) != 0
    for npal, p in ((0, 4), (1, 0), (1, big)):
        assert lib.wu_colour_ot_palette_keys(keys.ptr, npal, p, rot, keys.ptr, ws.data_ptr(), _stream()) != 0
    for b, h, w, nimg in ((1, 2, 2, 0), (0, 2, 2, 1), (1, 0, 2, 1), (1, 1, big, 1)):
        assert lib.wu_colour_ot_load(x.data_ptr(), *x.stride(), 0, b, h, w, 0.5, 0.5, 1.0, 0, nimg, state.ptr, _stream()) != 0
        assert lib.wu_colour_ot_store(state.ptr, 0, nimg, out.ptr, 12, 12, 4, 2, 1, 0, b, h, w, -1.0, 2.0, 0, _stream()) != 0
    assert lib.wu_colour_ot_load(x.data_ptr(), *x.stride(), 5, 1, 2, 2, 0.5, 0.5, 1.0, 0, 1, state.ptr, _stream()) != 0      # unknown dtype
    assert b"dtype" in lib.wu_last_error()
    torch.cuda.synchronize()
    for g, what in ((state, "state"), (keys, "keys"), (out, "out")):
        g.untouched(what)
    assert bool((ws == 0xFF).all())


def _write_pngs(directory, images_u8):
    from PIL import Image
    directory.mkdir()
    for i, im in enumerate(images_u8):
        Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0))).save(directory / f"im{i:02d}.png")


def test_palettes_from_directories_and_the_command_line(tmp_path, capsys):
    from PIL import Image
    from wu import colour
    src, snowy, rainy = CASES.images_u8(3, 24, 20, 91), CASES.images_u8(5, 24, 20, 92), CASES.noise_u8(4, 24, 20, 93)
    _write_pngs(tmp_path / "src", src)
    _write_pngs(tmp_path / "snowy", snowy)
    _write_pngs(tmp_path / "rainy", rainy)
    dirs = {"snowy": str(tmp_path / "snowy"), "rainy": str(tmp_path / "rainy")}
    pal = colour.ClassPalettes.from_dirs(dirs, P=300, seed=3, batch_size=2)
    assert pal.names == ["snowy", "rainy"] and pal.P == 300 and pal.seed == 3 and pal.sources == list(dirs.values())
    assert torch.equal(pal.palettes, colour.ClassPalettes.from_dirs(dirs, P=300, seed=3, batch_size=64).palettes)       # not the batch size
    for c, real in enumerate((snowy, rainy)):
        want = colour.palette_from_images(torch.from_numpy(real), 300, seed=3, value_range="uint8")
        assert np.array_equal(pal.palettes[c].cpu().numpy(), want.numpy())
    out = tmp_path / "out"
    rc = colour.main([str(tmp_path / "src"), str(out), "--class", f"snowy={dirs['snowy']}", "--class", f"rainy={dirs['rainy']}", "--iters", "3",
                      "--points", "300", "--seed", "3", "--save-palettes", str(tmp_path / "p.npz")])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Colour:")]
    assert len(line) == 1 and "3 images" in line[0] and "2 classes" in line[0] and "K 3" in line[0] and "P 300" in line[0]
    want = R.transfer(src, pal.palettes.cpu().numpy(), [0, 1], colour.draw_rotations(3, 3), 1.0, "uint8", _mapping("uint8"), "uint8")
    for c, name in enumerate(("snowy", "rainy")):
        files = sorted((out / name).iterdir())
        assert [f.name for f in files] == ["im00.png", "im01.png", "im02.png"]
        for i, f in enumerate(files):                                   # PNG is lossless: the bytes on disk are the transfer's bytes
            assert np.array_equal(np.asarray(Image.open(f).convert("RGB")).transpose(2, 0, 1), want[c, i]), (name, i)
    back = colour.ClassPalettes.load_npz(tmp_path / "p.npz")
    assert torch.equal(back.palettes, pal.palettes.cpu()) and back.names == pal.names
    out2 = tmp_path / "out2"
    assert colour.main([str(tmp_path / "src"), str(out2), "--palettes", str(tmp_path / "p.npz"), "--iters", "1", "--size", "32", "--ext",
                        ".jpg"]) == 0
    assert sorted(f.name for f in (out2 / "rainy").iterdir()) == ["im00.jpg", "im01.jpg", "im02.jpg"]
    assert Image.open(out2 / "snowy" / "im00.jpg").size == (32, 32)


class _NearestMean(torch.nn.Module):
    """A stand-in classifier: minus the squared distance of the image's mean colour to every class's mean colour."""

    def __init__(self, means):
        super().__init__()
        self.means = means

    def forward(self, x):
        m = x.float().mean(dim=(2, 3))
        return -((m[:, None, :] - self.means[None]) ** 2).sum(2)


def test_class_transfer_eval_takes_the_baseline():
    from wu import colour, evaluate
    nc = 3
    x = CASES.images(4, 32, 32, 81)
    pal = CASES.palettes(nc, 4096, seed=82)
    means = torch.from_numpy((pal.mean(1) * 2 - 1).astype(np.float32)).to(DEV)
    clf = _NearestMean(means)
    content = evaluate.ContentPreservation(ms=False)
    ev = evaluate.ClassTransferEval(colour.ColourBaseline(colour.ClassPalettes(pal), iters=5, seed=4), clf, nc, content=content)
    xd = torch.from_numpy(x).to(DEV)
    ev.update(xd)
    ev.update(xd.flip(0))
    want = R.transfer(x, pal, list(range(nc)), colour.draw_rotations(4, 5), 1.0, (-1, 1), _mapping((-1, 1)), "float32")
    pred = clf(torch.from_numpy(want).to(DEV).view(nc * 4, 3, 32, 32)).argmax(1).cpu().numpy()
    cm = np.zeros((nc, nc), dtype=np.int64)
    for t, q in zip(np.repeat(np.arange(nc), 4), pred):
        cm[t, q] += 2                        # the flipped batch holds the same images
    assert np.array_equal(ev.confusion().cpu().numpy(), cm)
    assert np.trace(cm) == 2 * nc * 4        # a colour classifier sees the target colours (the logits are 0.5 apart in the restatement)
    res = content.result()
    assert res["count"] == 8 and res["ssim"].shape == (nc,) and bool((res["ssim"] < 1).all())
