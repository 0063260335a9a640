"""Regraining and the linear colour maps on the GPU (csrc/colour_regrain.hip through the C ABI, wu.colour) against tests/_regrain_ref.py.

Everything is compared with np.array_equal: both sides do the same float64 operations in the same order without FMA, the sums of the
moments run in an order fixed by their length, and the Jacobi eigendecomposition has no trigonometry -- there is no tolerance anywhere.
Shapes: the degenerate 1 x 1, 1 x 7, 2 x 3 and 7 x 1; three levels of odd sizes; (150, 170), which is three owned tiles and a remainder
both ways at the deepest halo (8) and has a tiled second level; 42 x 42 (two levels) and 224 x 224 (four, the coarsest two in one launch
each) with the defaults.

ABI-level outputs live in tests/_gpu_guard.py buffers: guards on both sides checked after the call; workspaces start as 0xFF."""
import ctypes

import numpy as np
import pytest
import torch

import _colour_cases as CC
import _colour_ref as CR
import _regrain_cases as CASES
import _regrain_ref as G
from _gpu_guard import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.uint8: "uint8"}


def _lib():
    from wu import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class GuardedF64(Guarded):
    """n doubles inside a Guarded float buffer: two NaN floats side by side are a NaN double, and the payload starts 128 bytes in."""

    def __init__(self, n, init=None):
        super().__init__(2 * n)
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64).reshape(-1).view(np.float32)))

    def numpy(self, what, shape=None):
        out = super().numpy(what).view(np.float64)
        return out.reshape(shape) if shape is not None else out


def _mapping(value_range):
    from wu import paired
    return paired.range_mapping(value_range)


def _host(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _abi_regrain(i0, it, iters, min_side, smoothness):
    """i0, it (nimg, 3, h, w) float64 -> IR (nimg, 3, h, w) through wu_colour_regrain, every buffer guarded, the original checked unchanged."""
    L, lib = _lib()
    nimg, _, h, w = i0.shape
    levels = lib.wu_colour_regrain_levels(h, w, len(iters), min_side)
    assert levels == len(G.level_sizes(h, w, len(iters), min_side))
    nbytes = lib.wu_colour_regrain_workspace_bytes(nimg, h, w, levels)
    assert nbytes > 0
    ws = Guarded(nbytes // 4)
    ws.view.view(torch.uint8).fill_(0xFF)
    state, orig = GuardedF64(nimg * 3 * h * w, it), GuardedF64(nimg * 3 * h * w, i0)
    L.call("wu_colour_regrain", state.ptr, orig.ptr, nimg, h, w, levels, _ints(list(iters[:levels])), float(smoothness), ws.ptr, _stream())
    torch.cuda.synchronize()
    ws.numpy("wu_colour_regrain (workspace)")
    assert np.array_equal(orig.numpy("wu_colour_regrain (original)", i0.shape), i0), "original modified"
    return state.numpy("wu_colour_regrain (state)", i0.shape)


def _want_regrain(i0, it, iters, min_side, smoothness):
    return np.stack([G.regrain(i0[i], it[i], iters, smoothness, min_side) for i in range(i0.shape[0])])


@pytest.mark.parametrize("h,w,iters,min_side,smoothness", CASES.ABI_CASES + [(224, 224, G.DEFAULT_ITERS, 20, 1.0)])
def test_regrain_bit_exact_through_the_abi(h, w, iters, min_side, smoothness):
    nimg = 2
    i0, it = CASES.pair(nimg, h, w, seed=h + w)
    assert it.min() < 0.0 and it.max() > 1.0 or h * w < 8                    # the transfer reaches outside [0, 1]: nothing is clipped
    want = _want_regrain(i0, it, iters, min_side, smoothness)
    got = _abi_regrain(i0, it, iters, min_side, smoothness)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} values differ, max {np.abs(got - want).max():.3e}"
    if h * w > 8:
        assert np.abs(want - it).max() > 1e-3                                # the pass moved something: not a trivially-equal comparison


def test_images_of_a_call_do_not_mix_and_repeats_agree():
    i0, it = CASES.pair(3, 70, 66, seed=5)                                    # 4620 pixels: tiled at level 0, one region at level 1
    iters = (9, 5)
    whole = _abi_regrain(i0, it, iters, 0, 1.0)
    assert np.array_equal(whole, _abi_regrain(i0, it, iters, 0, 1.0))
    for i in range(3):
        assert np.array_equal(_abi_regrain(i0[i:i + 1], it[i:i + 1], iters, 0, 1.0)[0], whole[i])


def test_bad_arguments_are_refused_before_any_launch():
    L, lib = _lib()
    state, orig = GuardedF64(3 * 64), GuardedF64(3 * 64)
    ws = torch.full((1 << 16,), 0xFF, dtype=torch.uint8, device=DEV)
    big = (1 << 21) + 1

    def call(nimg=1, h=8, w=8, levels=1, iters=(2,), smoothness=1.0, st=state.ptr, og=orig.ptr, wp=None):
        return lib.wu_colour_regrain(st, og, nimg, h, w, levels, _ints(list(iters)) if iters is not None else None, smoothness,
                                     ws.data_ptr() if wp is None else wp, _stream())

    for kw in (dict(nimg=0), dict(h=0), dict(w=0), dict(h=1, w=big), dict(levels=0), dict(levels=7, iters=(1,) * 7), dict(iters=(0,)),
               dict(levels=2, iters=(2, -1)), dict(iters=((1 << 20) + 1,)), dict(smoothness=0.0), dict(smoothness=-1.0),
               dict(smoothness=float("inf")), dict(smoothness=float("nan")), dict(st=None), dict(og=None), dict(wp=0), dict(iters=None)):
        assert call(**kw) != 0, kw
        assert lib.wu_last_error()
    mom, smom = GuardedF64(24), GuardedF64(24)
    cls = torch.zeros(2, dtype=torch.int32, device=DEV)
    for nsets, n, sp, sc in ((0, 64, 1, 64), (65536, 64, 1, 64), (1, 0, 1, 0), (1, big, 1, big), (1, 64, 2, 64), (1, 64, 1, 63), (1, 64, 3, 2)):
        assert lib.wu_colour_moments(state.ptr, sp, sc, nsets, n, mom.ptr, ws.data_ptr(), _stream()) != 0
    assert lib.wu_colour_moments(None, 1, 64, 1, 64, mom.ptr, ws.data_ptr(), _stream()) != 0
    for nimg, n, npal, mode, eps in ((0, 64, 1, 0, 1e-10), (1, 0, 1, 0, 1e-10), (1, big, 1, 0, 1e-10), (1, 64, 0, 0, 1e-10), (1, 64, 1, 2, 1e-10),
                                     (1, 64, 1, -1, 1e-10), (1, 64, 1, 1, 0.0), (1, 64, 1, 1, float("nan"))):
        assert lib.wu_colour_linear_apply(state.ptr, nimg, n, smom.ptr, mom.ptr, npal, cls.data_ptr(), mode, eps, _stream()) != 0
    assert lib.wu_colour_linear_apply(state.ptr, 1, 64, smom.ptr, mom.ptr, 1, None, 0, 1e-10, _stream()) != 0
    torch.cuda.synchronize()
    for g, what in ((state, "state"), (orig, "original"), (mom, "moments"), (smom, "state moments")):
        g.untouched(what)
    assert bool((ws == 0xFF).all())


@pytest.mark.parametrize("n,p", [(1, 1), (100, 37), (4096, 4097), (4097, 255), (3 * 4096 + 5, 8193)])
def test_moments_and_linear_apply_through_the_abi(n, p):
    L, lib = _lib()
    npal = 2
    rng = np.random.RandomState(n + p)
    s0 = np.round(rng.uniform(-0.5, 1.5, (3, 3, n)) * 4096) / 4096
    pal = CC.palettes(npal, p, seed=n)
    classes = [1, 0, 7]                                                       # the last one has no palette: its image must stay as it is
    ws = torch.full((max(lib.wu_colour_moments_workspace_bytes(3, n), lib.wu_colour_moments_workspace_bytes(npal, p)),), 0xFF, dtype=torch.uint8,
                    device=DEV)
    state, ms, mt = GuardedF64(3 * 3 * n, s0), GuardedF64(3 * 12), GuardedF64(npal * 12)
    pal_d = torch.from_numpy(pal).to(DEV)
    cls = torch.tensor(classes, dtype=torch.int32, device=DEV)
    L.call("wu_colour_moments", pal_d.data_ptr(), 3, 1, npal, p, mt.ptr, ws.data_ptr(), _stream())          # (C, P, 3): interleaved
    L.call("wu_colour_moments", state.ptr, 1, n, 3, n, ms.ptr, ws.data_ptr(), _stream())                    # (nimg, 3, n): planar
    got_ms, got_mt = ms.numpy("wu_colour_moments (state)", (3, 12)), mt.numpy("wu_colour_moments (palettes)", (npal, 12))
    want_s = [G.moments(s0[i]) for i in range(3)]
    want_t = [G.moments(np.ascontiguousarray(pal[c].T)) for c in range(npal)]
    for got, want in ((got_ms, want_s), (got_mt, want_t)):
        for row, (mu, cov) in zip(got, want):
            assert np.array_equal(row[:3], mu) and np.array_equal(row[3:].reshape(3, 3), cov)
    for mode, method in ((0, "meanstd"), (1, "mkl")):
        st = GuardedF64(3 * 3 * n, s0)
        L.call("wu_colour_linear_apply", st.ptr, 3, n, ms.ptr, mt.ptr, npal, cls.data_ptr(), mode, 1e-10, _stream())
        got = st.numpy(f"wu_colour_linear_apply ({method})", (3, 3, n))
        assert np.array_equal(got[0], G.linear_apply(s0[0], want_s[0], want_t[1], method)), method
        assert np.array_equal(got[1], G.linear_apply(s0[1], want_s[1], want_t[0], method)), method
        assert np.array_equal(got[2], s0[2]), method
    assert np.isfinite(got).all()
    ms.numpy("state moments after the applies"), mt.numpy("palette moments after the applies")


def _input_kinds(n, h, w, seed):
    """(name, CUDA tensor of some layout, the values the kernel must see as a numpy array, value_range): the four of test_gpu_colour.py; the
    padding of the cropped view is 0xFF bytes (a NaN as float32), which no kernel may read."""
    x = CC.images(n, h, w, seed)
    yield "float32 NCHW", torch.from_numpy(x).to(DEV), x, (-1, 1)
    xb = torch.from_numpy(x).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    yield "bf16 channels-last", xb, xb.float().cpu().numpy(), (-1, 1)
    u = CC.images_u8(n, h, w, seed + 1)
    ud = torch.from_numpy(np.ascontiguousarray(u.transpose(0, 2, 3, 1))).to(DEV).permute(0, 3, 1, 2)
    assert ud.stride(1) == 1 and not ud.is_contiguous()
    yield "uint8 NHWC view", ud, u, "uint8"
    inner = CC.images(n, h, w, seed + 2) * 0.5 + 0.5
    big = torch.full((n * 3 * (h + 5) * (w + 7) * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).view(n, 3, h + 5, w + 7)
    big[:, :, 2:2 + h, 3:3 + w] = torch.from_numpy(inner).to(DEV)
    crop = big[:, :, 2:2 + h, 3:3 + w]
    assert crop.storage_offset() > 0 and not crop.is_contiguous()
    yield "cropped view in 0xFF padding", crop, inner, (0, 1)


REGRAINS = {"idt": dict(iters=(4, 8), smoothness=1.0, min_side=10), "meanstd": dict(iters=(3,), smoothness=4.0, min_side=20),
            "mkl": dict(iters=G.DEFAULT_ITERS, smoothness=1.0, min_side=20)}


@pytest.mark.parametrize("method", ["idt", "meanstd", "mkl"])
def test_transfer_with_regraining_on_every_input_kind(method):
    from wu import colour
    b, h, w, targets, k, seed = 2, 48, 40, [1, 0, 1], 2, 3
    pal = CC.palettes(2, 777, seed=21)
    cp = colour.ClassPalettes(pal)
    kw = REGRAINS[method]
    rg = True if kw["iters"] == G.DEFAULT_ITERS else colour.Regrain(**kw)
    rots = colour.draw_rotations(seed, k)
    for name, xd, seen, value_range in _input_kinds(b, h, w, seed=h + w):
        want = G.transfer(seen, pal, targets, rots, 1.0, value_range, _mapping(value_range), NAMES[xd.dtype], method, kw)
        plain = G.transfer(seen, pal, targets, rots, 1.0, value_range, _mapping(value_range), NAMES[xd.dtype], method, None)
        assert not np.array_equal(want, plain), name
        before = xd.clone()
        got = colour.transfer(xd, cp, targets, k, seed, 1.0, value_range, None, method, rg)
        assert got.dtype == xd.dtype and tuple(got.shape) == (len(targets),) + tuple(xd.shape), name
        assert np.array_equal(_host(got), want), f"{name}: {(_host(got) != want).sum()} of {want.size} values differ"
        assert torch.equal(xd, before), f"{name}: input modified"
        for max_images in (1, 2, 100):
            assert torch.equal(colour.transfer(xd, cp, targets, k, seed, 1.0, value_range, max_images, method, rg), got), (name, max_images)
        assert torch.equal(colour.transfer(xd, cp, targets, k, seed, 1.0, value_range, None, method, rg), got), name
        got_plain = colour.transfer(xd, cp, targets, k, seed, 1.0, value_range, 4, method)
        assert np.array_equal(_host(got_plain), plain), f"{name}: without regraining"
        assert torch.equal(got[0], got[2])                                    # repeated targets agree


def test_regrain_on_a_sweep_shaped_non_contiguous_tensor():
    from wu import colour
    r, b, h, w = 3, 2, 33, 50
    x = CC.images(b, h, w, 71)
    y = np.clip(CC.images(r * b, h, w, 72).reshape(r, b, 3, h, w) * 0.3 + x[None, :, ::-1] * 0.7, -1, 1)
    xd = torch.from_numpy(x).to(DEV)
    yd = torch.from_numpy(np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))).to(DEV).to(torch.bfloat16).permute(1, 0, 2, 3, 4)
    assert tuple(yd.shape) == (r, b, 3, h, w) and not yd.is_contiguous()
    seen_y = yd.float().cpu().numpy()
    kw = dict(iters=(3, 5, 7), smoothness=2.0, min_side=4)
    want = G.regrain_images(x, seen_y, (-1, 1), _mapping((-1, 1)), "bfloat16", **kw)
    got = colour.regrain(xd, yd, (-1, 1), **kw)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (r, b, 3, h, w)
    assert np.array_equal(_host(got), want) and not np.array_equal(want, seen_y)
    assert torch.equal(colour.regrain(xd, yd, (-1, 1), max_images=1, **kw), got)
    one = colour.regrain(xd, yd[1], (-1, 1), **kw)                            # (B, 3, H, W) against (B, 3, H, W)
    assert tuple(one.shape) == (b, 3, h, w) and torch.equal(one, got[1])
    u = CC.images_u8(b, h, w, 73)
    ud = torch.from_numpy(u).to(DEV)
    got_u = colour.regrain(ud, ud.flip(1), "uint8")
    assert got_u.dtype == torch.uint8
    assert np.array_equal(got_u.cpu().numpy(), G.regrain_images(u, u[:, ::-1], "uint8", _mapping("uint8"), "uint8"))


@pytest.mark.parametrize("h,w,p,b,targets,k,step", [(1, 7, 22, 1, [0, 1, 2], 5, 0.5), (48, 40, 3 * 48 * 40 + 1, 2, [2, 0, 1], 5, 1.0)])
def test_defaults_are_unchanged(h, w, p, b, targets, k, step):
    from wu import colour
    x = CC.images(b, h, w, seed=h + w + p)
    pal = CC.palettes(3, p, seed=p + k)
    want = CR.transfer(x, pal, targets, colour.draw_rotations(k + 1, k), step, (-1, 1), _mapping((-1, 1)), "float32")
    xd, cp = torch.from_numpy(x).to(DEV), colour.ClassPalettes(pal)
    old = colour.transfer(xd, cp, targets, k, k + 1, step, (-1, 1))
    new = colour.transfer(xd, cp, targets, k, k + 1, step, (-1, 1), method="idt", regrain=None)
    assert np.array_equal(old.cpu().numpy(), want) and torch.equal(old, new)
    assert torch.equal(colour.ColourBaseline(cp, k, k + 1).sweep(xd, torch.eye(3)[targets]), old) or step != 1.0


def _write_pngs(directory, images_u8):
    from PIL import Image
    directory.mkdir()
    for i, im in enumerate(images_u8):
        Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0))).save(directory / f"im{i:02d}.png")


def test_command_line_routes(tmp_path, capsys):
    from PIL import Image
    from wu import colour
    from wu.infer_driver import save_images
    src, snowy, rainy = CC.images_u8(4, 16, 12, 91), CC.images_u8(5, 16, 12, 92), CC.noise_u8(4, 16, 12, 93)
    _write_pngs(tmp_path / "src", src)
    _write_pngs(tmp_path / "snowy", snowy)
    _write_pngs(tmp_path / "rainy", rainy)
    dirs = {"snowy": str(tmp_path / "snowy"), "rainy": str(tmp_path / "rainy")}
    routes = [(["--class", f"snowy={dirs['snowy']}", "--class", f"rainy={dirs['rainy']}", "--points", "150", "--seed", "3", "--save-palettes",
                str(tmp_path / "p.npz"), "--method", "mkl", "--regrain"], "mkl", dict(), "method mkl", "regrain on"),
              (["--palettes", str(tmp_path / "p.npz"), "--method", "meanstd", "--regrain-smoothness", "4"], "meanstd", dict(smoothness=4.0),
               "method meanstd", "smoothness 4"),
              (["--palettes", str(tmp_path / "p.npz"), "--iters", "2", "--seed", "3"], "idt", None, "K 2", "regrain off")]
    for i, (argv, method, kw, *marks) in enumerate(routes):
        out = tmp_path / f"out{i}"
        assert colour.main([str(tmp_path / "src"), str(out)] + argv) == 0
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Colour:")]
        assert len(line) == 1 and "4 images" in line[0] and "2 classes" in line[0] and "P 150" in line[0] and all(m in line[0] for m in marks)
        pal = colour.ClassPalettes.load_npz(tmp_path / "p.npz")
        want = G.transfer(src, pal.palettes.numpy(), [0, 1], colour.draw_rotations(3, 2), 1.0, "uint8", _mapping("uint8"), "uint8", method, kw)
        for c, name in enumerate(("snowy", "rainy")):
            files = sorted((out / name).iterdir())
            assert [f.name for f in files] == [f"im{j:02d}.png" for j in range(4)]
            # the restatement's bytes through the same writer: the files must be identical, and hold those bytes
            ref = tmp_path / f"ref{i}_{name}"
            ref.mkdir()
            w01 = (torch.from_numpy(want[c]).to(DEV).float() + 0.5) / 255
            save_images(w01, [str(ref / f.name) for f in files], normalize=False)
            for j, f in enumerate(files):
                assert f.read_bytes() == (ref / f.name).read_bytes(), (method, name, j)
                assert np.array_equal(np.asarray(Image.open(f).convert("RGB")).transpose(2, 0, 1), want[c, j]), (method, name, j)


class _NearestMean(torch.nn.Module):
    """A stand-in classifier: minus the squared distance of the image's mean colour to every class's mean colour."""

    def __init__(self, means):
        super().__init__()
        self.means = means

    def forward(self, x):
        m = x.float().mean(dim=(2, 3))
        return -((m[:, None, :] - self.means[None]) ** 2).sum(2)


def test_class_transfer_eval_takes_the_regrained_linear_baseline():
    from wu import colour, evaluate
    nc = 3
    x = CC.images(4, 32, 32, 81)
    pal = CC.palettes(nc, 4096, seed=82)
    means = torch.from_numpy((pal.mean(1) * 2 - 1).astype(np.float32)).to(DEV)
    clf = _NearestMean(means)
    content = evaluate.ContentPreservation(ms=False)
    ev = evaluate.ClassTransferEval(colour.ColourBaseline(colour.ClassPalettes(pal), method="mkl", regrain=True), clf, nc, content=content)
    xd = torch.from_numpy(x).to(DEV)
    ev.update(xd)
    ev.update(xd.flip(0))
    want = G.transfer(x, pal, list(range(nc)), None, 1.0, (-1, 1), _mapping((-1, 1)), "float32", "mkl", dict())
    pred = clf(torch.from_numpy(want).to(DEV).view(nc * 4, 3, 32, 32)).argmax(1).cpu().numpy()
    cm = np.zeros((nc, nc), dtype=np.int64)
    for t, q in zip(np.repeat(np.arange(nc), 4), pred):
        cm[t, q] += 2                        # the flipped batch holds the same images
    assert np.array_equal(ev.confusion().cpu().numpy(), cm)
    assert np.trace(cm) == 2 * nc * 4        # the linear map takes the mean colour to the palette's: a colour classifier sees the target
    res = content.result()
    assert res["count"] == 8 and res["ssim"].shape == (nc,) and bool((res["ssim"] < 1).all())
