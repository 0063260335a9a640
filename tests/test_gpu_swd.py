"""Sliced Wasserstein distance on the GPU (csrc/swd.hip through the C ABI, wu.swd and wu.evaluate.SlicedWasserstein) against
tests/_swd_ref.py, stage by stage.

* Pyramid and gather: the float32 descriptors EQUAL the restatement's (same fp64 operations in the same order, no FMA).
* Statistics: mu / sigma within 49 m 2^-53 relative of numpy's float64 (non-negative terms, or terms of one sign, summed in any order);
  with the GPU's own mu / sigma fed to the restatement the normalised float32 descriptors are equal.
* Sort: with integer descriptors and one-hot directions every projection is exactly a descriptor column, so the sorted columns equal
  np.sort.
* Projection and distance: a projection is a 147-term inner product in fp64, off by at most 147 2^-53 |d| |dir| in either implementation;
  sorting is 1-Lipschitz in the sup norm and |a - b| sees two columns, so |w_j - ref_j| <= 4 * 147 * 2^-53 * R with R the largest
  descriptor row 2-norm of the case, computed from the data.  (The end-to-end case applies the same bound although its two sides normalise
  with statistics that agree to rounding only: a float32 rounding flip there would need a quotient within 1e-16 of a rounding boundary.)

Outputs live in tests/_gpu_guard.py buffers: NaN before the call, guards on both sides checked after it."""
import functools

import numpy as np
import pytest
import torch

import _swd_cases as CASES
import _swd_ref as R
from _gpu_guard import Guarded, Input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}


def _lib():
    from wu import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _block():
    return _lib()[1].wu_swd_sort_block()


class GuardedF64(Guarded):
    """n doubles inside a Guarded float buffer: two NaN floats side by side are a NaN double, and the payload starts 128 bytes in."""

    def __init__(self, n):
        super().__init__(2 * n)

    def numpy(self, what, shape=None):
        out = super().numpy(what).view(np.float64)
        return out.reshape(shape) if shape is not None else out


# ---------------------------------------------------------------------------------------------------------------------------------
# pyramid and gather
# ---------------------------------------------------------------------------------------------------------------------------------
def _abi_descriptors(x, pos, scale, shift, levels):
    L, lib = _lib()
    n, _, h, w = x.shape
    p = pos.shape[2]
    nbytes = lib.wu_swd_pyramid_workspace_bytes(n, h, w, levels, p)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    pos_d = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int32)).to(DEV)
    out = Guarded(levels * n * p * 147)
    L.call("wu_swd_descriptors", x.data_ptr(), *x.stride(), CODES[x.dtype], n, h, w, scale, shift, levels, pos_d.data_ptr(), p,
           ws.data_ptr(), out.ptr, _stream())
    torch.cuda.synchronize()
    return out.numpy("wu_swd_descriptors", (levels, n * p, 147))


def _input_kinds(n, h, w, seed):
    """(name, CUDA tensor of some layout, the values the kernel must see as a numpy array, value_range)."""
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


@pytest.mark.parametrize("n,p", CASES.GATHER_NP)
@pytest.mark.parametrize("h,w,levels", CASES.GATHER_SHAPES)
def test_descriptors_bit_exact(h, w, levels, n, p):
    from wu import paired, swd
    pos = CASES.positions(n, p, h, w, levels, seed=h + w + n + p)
    if n * p >= 4:
        for l, (hl, wl) in enumerate(CASES.level_shapes(h, w, levels)):
            flat = pos[l].reshape(-1, 2).tolist()
            assert [3, 3] in flat and [hl - 4, wl - 4] in flat and [3, wl - 4] in flat and [hl - 4, 3] in flat
    for name, xd, seen, value_range in _input_kinds(n, h, w, seed=7 * h + levels):
        scale, shift, _ = paired.range_mapping(value_range)
        want = R.descriptors(seen, pos, scale, shift, levels)
        got = _abi_descriptors(xd, pos, scale, shift, levels)
        for l in range(levels):
            assert np.array_equal(got[l], want[l]), f"{name}: level {l} differs in {(got[l] != want[l]).sum()} of {want[l].size} values"
        if levels > 1:
            assert np.abs(want[0]).max() > 0.01                     # a Laplacian level with signal, not a trivially-zero comparison
        via = swd.descriptors(xd, pos, value_range, levels)
        assert len(via) == levels and via[0].shape == (n * p, 147) and via[0].dtype == torch.float32 and via[0].is_cuda
        assert all(np.array_equal(via[l].cpu().numpy(), want[l]) for l in range(levels)), name


def test_descriptors_reject_positions_outside_the_bounds():
    from wu import swd
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    for bad in ((2, 3), (3, 13), (13, 3)):
        with pytest.raises(ValueError, match="position"):
            swd.descriptors(x, np.array(bad, dtype=np.int32).reshape(1, 1, 1, 2), levels=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics and normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
def _abi_normalize(desc):
    L, lib = _lib()
    m = desc.shape[0]
    src = Input(desc)
    nbytes = lib.wu_swd_stats_workspace_bytes(m)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out, stats = Guarded(m * 147), GuardedF64(6)
    L.call("wu_swd_normalize", src.ptr, m, ws.data_ptr(), out.ptr, stats.ptr, _stream())
    torch.cuda.synchronize()
    src.unchanged("wu_swd_normalize")
    st = stats.numpy("wu_swd_normalize stats")
    return out.numpy("wu_swd_normalize", (m, 147)), st[:3], st[3:]


@pytest.mark.parametrize("m", [1, 100, 64 * 1024 + 5, 70001])
def test_statistics_and_normalisation(m):
    """Values of one sign per channel (offsets 1, 2, 3), so that 'relative' is relative to the number itself."""
    rng = np.random.RandomState(m)
    desc = (rng.uniform(-0.5, 0.5, (m, 3, 49)) * np.array([0.1, 1.0, 0.4])[None, :, None] + np.array([1.0, 2.0, 3.0])[None, :, None])
    desc = desc.astype(np.float32).reshape(m, 147)
    got, mu, sigma = _abi_normalize(desc)
    mu_ref, sigma_ref = R.statistics(desc)
    bound = 49 * m * U
    print(f"m {m}: mu rel err {np.abs(mu - mu_ref) / np.abs(mu_ref)}, sigma rel err {np.abs(sigma - sigma_ref) / sigma_ref}, bound {bound:.3e}")
    assert np.all(np.abs(mu - mu_ref) <= bound * np.abs(mu_ref))
    assert np.all(np.abs(sigma - sigma_ref) <= bound * sigma_ref)
    want = R.normalize(desc, mu, sigma)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} normalised values differ"


def test_constant_channel_comes_out_zero():
    from wu import swd
    rng = np.random.RandomState(0)
    desc = rng.randn(300, 147).astype(np.float32)
    desc[:, 49:98] = 0.625
    desc[:, 98:] = 0.0
    got, mu, sigma = _abi_normalize(desc)
    assert mu[1] == 0.625 and mu[2] == 0.0 and sigma[1] == 0.0 and sigma[2] == 0.0 and sigma[0] > 0
    assert np.all(got[:, 49:] == 0) and np.isfinite(got).all()
    assert np.array_equal(got, R.normalize(desc, mu, sigma))
    dn, mu_t, sigma_t = swd.normalize(torch.from_numpy(desc).to(DEV))
    assert np.array_equal(dn.cpu().numpy(), got) and np.array_equal(mu_t.cpu().numpy(), mu) and np.array_equal(sigma_t.cpu().numpy(), sigma)


# ---------------------------------------------------------------------------------------------------------------------------------
# projection and sort
# ---------------------------------------------------------------------------------------------------------------------------------
def _abi_sorted(desc, dirs, dir_chunk=0):
    L, lib = _lib()
    m, nd = desc.shape[0], dirs.shape[0]
    a, b = Input(desc), Input(dirs)
    nbytes = lib.wu_swd_workspace_bytes(m, nd, dir_chunk)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = GuardedF64(nd * m)
    L.call("wu_swd_project_sort", a.ptr, m, b.ptr, nd, dir_chunk, ws.data_ptr(), out.ptr, _stream())
    torch.cuda.synchronize()
    a.unchanged("wu_swd_project_sort")
    b.unchanged("wu_swd_project_sort")
    return out.numpy("wu_swd_project_sort", (nd, m))


def _sort_size(index):
    return CASES.sort_sizes(_block())[index]


@pytest.mark.parametrize("index", range(10))
def test_sort_is_exact(index):
    """m = 1, 2, 63, 64, 65, b - 1, b, b + 1, 2 b + 17, 5 b + 3 (b = wu_swd_sort_block()); 70 directions (not a multiple of the 64-wide
    tile) up to b + 1 keys and 5 above; every kind of input, each with another dir_chunk."""
    m = _sort_size(index)
    ncols = 70 if m <= _block() + 1 else 5
    for kind, chunk in zip(CASES.SORT_KINDS, (0, 1, 3, 64, ncols)):
        desc, dirs, cols = CASES.one_hot_case(m, ncols, kind, seed=index)
        got = _abi_sorted(desc, dirs, chunk)
        want = np.sort(cols.astype(np.float64), axis=0).T
        assert (cols < 0).any() or kind == "ascending" and m == 1
        assert np.array_equal(got, want), f"m {m} {kind} dir_chunk {chunk}: {(got != want).sum()} of {want.size} keys differ"


@pytest.mark.parametrize("which", ["3", "b", "b+1", "3b+5"])
def test_sort_columns_alone(which):
    """The sort without the projection in front of it, on doubles that are no integers: in place, an odd and an even number of merge
    passes (the odd one ends in the workspace and is copied back)."""
    from wu import swd
    b = _block()
    m = {"3": 3, "b": b, "b+1": b + 1, "3b+5": 3 * b + 5}[which]
    keys = np.random.RandomState(m).randn(7, m) * np.array([1e-300, 1.0, 1e300, 1.0, 3.0, 1e-5, 1.0])[:, None]
    keys[3] = np.round(keys[3] * 4) / 4
    buf = GuardedF64(7 * m)
    view = buf.view.view(torch.float64).view(7, m)
    view.copy_(torch.from_numpy(keys))
    assert swd.sort_columns(view) is view
    torch.cuda.synchronize()
    assert np.array_equal(buf.numpy("wu_swd_sort_columns", (7, m)), np.sort(keys, axis=1))


def _abi_distance(a, b):
    L, lib = _lib()
    nd, m = a.shape
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    w = GuardedF64(nd)
    L.call("wu_swd_distance", ad.data_ptr(), bd.data_ptr(), m, nd, w.ptr, _stream())
    torch.cuda.synchronize()
    return w.numpy("wu_swd_distance")


def _bound(*descs):
    r = max(np.sqrt(np.square(d.astype(np.float64)).sum(axis=1)).max() for d in descs)
    return 4 * 147 * U * r


@pytest.mark.parametrize("which", ["1", "100", "b+1"])
def test_projection_and_distance(which):
    m = {"1": 1, "100": 100, "b+1": _block() + 1}[which]
    d1, d2 = CASES.normalised_descriptors(m, 11), 0.8 * CASES.normalised_descriptors(m, 12) + 0.1
    d2 = d2.astype(np.float32)
    dirs = CASES.unit_dirs(70, 13)
    a, b = _abi_sorted(d1, dirs), _abi_sorted(d2, dirs, 7)
    assert np.all(np.diff(a, axis=1) >= 0) and np.all(np.diff(b, axis=1) >= 0)
    bound = _bound(d1, d2)
    ra, rb = R.sorted_projections(d1, dirs), R.sorted_projections(d2, dirs)
    print(f"m {m}: sorted projections off by {max(np.abs(a - ra).max(), np.abs(b - rb).max()):.3e}, bound {bound / 2:.3e}")
    assert np.abs(a - ra).max() <= bound / 2 and np.abs(b - rb).max() <= bound / 2          # 2 * 147 u R per column
    w = _abi_distance(a, b)
    ref = R.sliced_wasserstein(d1, d2, dirs)
    print(f"m {m}: |w - ref| max {np.abs(w - ref).max():.3e}, bound {bound:.3e}, w in [{ref.min():.4f}, {ref.max():.4f}]")
    assert ref.min() > 0 and np.all(np.abs(w - ref) <= bound)
    from wu import swd
    via = swd.sliced_wasserstein(torch.from_numpy(d1).to(DEV), torch.from_numpy(d2).to(DEV), dirs)
    assert via.dtype == torch.float64 and via.is_cuda and np.array_equal(via.cpu().numpy(), w)


def test_distance_kernel_alone():
    """Integers: the sum is exact in any order."""
    rng = np.random.RandomState(5)
    for m in (1, 255, 256, 257, 5000):
        a, b = rng.randint(-50, 50, (3, m)).astype(np.float64), rng.randint(-50, 50, (3, m)).astype(np.float64)
        assert np.array_equal(_abi_distance(a, b), np.abs(a - b).sum(axis=1) / m)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e():
    x, y = CASES.images(4, 32, 32, 21), CASES.images(4, 32, 32, 22)
    y = (0.7 * y + 0.1 * np.random.RandomState(23).uniform(-1, 1, y.shape)).astype(np.float32)
    return x, y, torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)


def test_swd_end_to_end():
    from wu import swd
    x, y, xd, yd = _e2e()
    r = swd.swd(xd, yd, P=8, repeats=2, dirs_per_repeat=8, seed=4)
    assert swd.default_levels(32, 32) == 2 and len(r.levels) == 2
    pos, dirs = swd.draw(4, 2, [(32, 32), (16, 16)], 4, 8, 16)
    want = R.swd_levels(x, y, pos, dirs, 0.5, 0.5, 2)
    da, db = R.descriptors(x, pos, 0.5, 0.5, 2), R.descriptors(y, pos, 0.5, 0.5, 2)
    for l in range(2):
        bound = _bound(R.normalize(da[l]), R.normalize(db[l]))
        print(f"level {l}: swd {r.levels[l] / 1e3:.6f} ref {want[l]:.6f} diff {abs(r.levels[l] / 1e3 - want[l]):.3e} bound {bound:.3e}")
        assert want[l] > 1e-3 and abs(r.levels[l] / 1e3 - want[l]) <= bound
    assert r.mean == pytest.approx(np.mean(r.levels), rel=1e-15)


def test_swd_of_a_set_with_itself_is_zero_and_runs_repeat():
    from wu import swd
    _, _, xd, yd = _e2e()
    r = swd.swd(xd, xd.clone(), P=8, repeats=2, dirs_per_repeat=8)
    assert r.levels == (0.0, 0.0) and r.mean == 0.0
    first = swd.swd(xd, yd, P=8, repeats=2, dirs_per_repeat=8)
    assert swd.swd(xd, yd, P=8, repeats=2, dirs_per_repeat=8) == first
    for chunk in (1, 3):
        assert swd.swd(xd, yd, P=8, repeats=2, dirs_per_repeat=8, dir_chunk=chunk) == first
    assert swd.swd(xd, yd, P=8, repeats=2, dirs_per_repeat=8, seed=1) != first


def test_unequal_sets_raise():
    from wu import swd
    _, _, xd, yd = _e2e()
    with pytest.raises(ValueError, match="unequal"):
        swd.swd(xd, yd[:3], P=8)
    with pytest.raises(ValueError, match="unequal"):
        swd.sliced_wasserstein(torch.zeros(5, 147, device=DEV), torch.zeros(4, 147, device=DEV), CASES.unit_dirs(4, 0))
    with pytest.raises(ValueError, match="smaller"):
        swd.swd(xd, yd, levels=4)                                       # 32 / 8 = 4 < 7
    with pytest.raises(ValueError, match="divisible"):
        swd.swd(xd[..., :31, :], yd[..., :31, :], levels=2)
    with pytest.raises(ValueError, match="at least 1"):
        swd.swd(xd[..., :8, :8], yd[..., :8, :8])                       # below 16: no default level


# ---------------------------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_accumulator_in_two_batches_equals_one_call():
    from wu import swd
    from wu.evaluate import SlicedWasserstein
    _, _, xd, yd = _e2e()
    whole = swd.swd(xd, yd, P=8, repeats=2, dirs_per_repeat=8, seed=9)
    acc = SlicedWasserstein(P=8, repeats=2, dirs_per_repeat=8, seed=9)
    acc.update(xd[:3], yd[:3])
    acc.update(xd[3:], yd[3:])
    assert acc.compute() == whole
    rows = SlicedWasserstein(P=8, repeats=2, dirs_per_repeat=8, seed=9)
    rows.update(xd[:1], torch.stack([yd[:1], xd[:1]]))
    rows.update(xd[1:], torch.stack([yd[1:], xd[1:]]))
    got = rows.compute()
    assert isinstance(got, list) and got[0] == whole and got[1].mean == 0.0


class _Sweep:
    """A stand-in generator: row r of the sweep is the batch scaled by a class-dependent gain."""

    def sweep(self, batch, rows, max_images):
        gains = 1.0 - 0.1 * torch.arange(rows.shape[0], device=batch.device, dtype=batch.dtype)
        return batch.unsqueeze(0) * gains.view(-1, 1, 1, 1, 1)


def _classifier(images):
    return torch.stack([images.mean((1, 2, 3)), images.amax((1, 2, 3)), images.amin((1, 2, 3))], 1)


def test_transfer_evaluations_take_swd_and_default_to_none():
    from wu.evaluate import ClassTransferEval, EstimatorTransferEval, SlicedWasserstein
    _, _, xd, _ = _e2e()
    plain = ClassTransferEval(_Sweep(), _classifier, 3)
    none = ClassTransferEval(_Sweep(), _classifier, 3, swd=None)
    acc = SlicedWasserstein(P=8, repeats=2, dirs_per_repeat=8)
    with_swd = ClassTransferEval(_Sweep(), _classifier, 3, swd=acc)
    for ev in (plain, none, with_swd):
        ev.update(xd[:2])
        ev.update(xd[2:])
    assert plain.swd is None and torch.equal(plain.confusion(), none.confusion()) and torch.equal(plain.confusion(), with_swd.confusion())
    assert plain.report() == none.report()
    per_class = acc.compute()
    assert len(per_class) == 3 and per_class[0].mean == 0.0 and len(per_class[1].levels) == 2     # gain 1: the photographs themselves
    est_acc = SlicedWasserstein(P=8, repeats=2, dirs_per_repeat=8)
    est = EstimatorTransferEval(_Sweep(), _classifier, swd=est_acc)
    ref = EstimatorTransferEval(_Sweep(), _classifier)
    for ev in (est, ref):
        ev.update(xd, torch.eye(3)[:2])
    assert torch.equal(est.result()["mean"], ref.result()["mean"]) and len(est_acc.compute()) == 2


def test_command_line(tmp_path, capsys):
    """Two directories of unequal count: a seeded subset of the larger one, announced; the printed values are swd() of the images used.
    Then mixed sizes: an error without --size, one size through wu.input_pipeline with it."""
    from PIL import Image
    from wu import swd
    from wu.fid import image_files
    a, b = CASES.images_u8(5, 32, 32, 31), CASES.images_u8(7, 32, 32, 32)
    for name, arr in (("a", a), ("b", b)):
        (tmp_path / name).mkdir()
        for i, img in enumerate(arr):
            Image.fromarray(img.transpose(1, 2, 0)).save(tmp_path / name / f"{i:02d}.png")
    assert swd.main([str(tmp_path / "a"), str(tmp_path / "b"), "--patches", "8", "--repeats", "2", "--dirs", "8", "--seed", "3"]) == 0
    out = capsys.readouterr().out
    assert "random subset" in out and "5 images per set" in out and "images per set: 5" in out
    keep = sorted(np.random.RandomState(3).permutation(7)[:5].tolist())
    want = swd.swd(torch.from_numpy(a).to(DEV), torch.from_numpy(b[keep]).to(DEV), P=8, repeats=2, dirs_per_repeat=8, seed=3,
                   value_range="uint8")
    lines = [ln for ln in out.splitlines() if ln.startswith("SWD")]
    assert lines == [f"SWD x 1e3, level {l}: {v:.4f}" for l, v in enumerate(want.levels)] + [f"SWD x 1e3, mean: {want.mean:.4f}"]
    assert len(image_files(str(tmp_path / "b"))) == 7
    Image.fromarray(CASES.images_u8(1, 40, 36, 33)[0].transpose(1, 2, 0)).save(tmp_path / "a" / "99.png")
    with pytest.raises(ValueError, match="--size"):
        swd.main([str(tmp_path / "a"), str(tmp_path / "b"), "--patches", "8", "--repeats", "1", "--dirs", "8"])
    capsys.readouterr()
    assert swd.main([str(tmp_path / "a"), str(tmp_path / "b"), "--size", "32", "--patches", "8", "--repeats", "1", "--dirs", "8"]) == 0
    out = capsys.readouterr().out
    assert "images per set: 6" in out and out.count("SWD x 1e3, level") == 2


def test_out_of_range_arguments_are_rejected_without_a_launch():
    L, lib = _lib()
    desc, dirs = Input(np.zeros((4, 147))), Input(np.zeros((2, 147)))
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    out = GuardedF64(64)
    for m, nd, chunk in (((1 << 21) + 1, 2, 0), (0, 2, 0), (4, 4097, 0), (4, 0, 0), (4, 2, -1)):
        assert lib.wu_swd_workspace_bytes(m, nd, chunk) == 0
        assert lib.wu_swd_project_sort(desc.ptr, m, dirs.ptr, nd, chunk, ws.data_ptr(), out.ptr, _stream()) < 0
        assert b"wu_swd_project_sort" in lib.wu_last_error()
    assert lib.wu_swd_distance(ws.data_ptr(), ws.data_ptr(), 4, 4097, out.ptr, _stream()) < 0
    assert lib.wu_swd_distance(ws.data_ptr(), ws.data_ptr(), (1 << 21) + 1, 2, out.ptr, _stream()) < 0
    torch.cuda.synchronize()
    out.untouched("wu_swd_project_sort / wu_swd_distance")
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    pos = torch.full((3, 1, 1, 2), 3, dtype=torch.int32, device=DEV)
    dout = Guarded(3 * 147)
    for levels in (0, 13, 4):                      # 32 / 8 = 4 < 7
        assert lib.wu_swd_pyramid_workspace_bytes(1, 32, 32, levels, 1) == 0
        rc = lib.wu_swd_descriptors(x.data_ptr(), *x.stride(), 0, 1, 32, 32, 1.0, 0.0, levels, pos.data_ptr(), 1, ws.data_ptr(), dout.ptr, _stream())
        assert rc < 0 and b"levels" in lib.wu_last_error()
    nout = Guarded(147)
    assert lib.wu_swd_normalize(desc.ptr, 0, ws.data_ptr(), nout.ptr, out.ptr, _stream()) < 0
    torch.cuda.synchronize()
    dout.untouched("wu_swd_descriptors")
    nout.untouched("wu_swd_normalize")
    out.untouched("wu_swd_normalize stats")
    from wu import swd
    with pytest.raises(ValueError, match="out of range"):
        swd.sorted_projections(torch.zeros(4, 147, device=DEV), torch.zeros(4097, 147, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        swd.swd(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))
