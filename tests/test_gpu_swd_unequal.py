"""The sliced Wasserstein distance between sets of unequal size on the GPU: wu_swd_distance_unequal through the C ABI, then
``unequal="exact"`` through wu.swd, wu.swd.DescriptorBank / compare, wu.evaluate.SlicedWasserstein(reference=) and the command line,
against tests/_swd_unequal_ref.py (the closed form in numpy, itself pinned to rational arithmetic by tests/test_swd_unequal_cpu.py) chained
onto tests/_swd_ref.py.

* Kernel alone, integer keys: weights, differences and products are integers and the sum stays below 2^53, so it is exact in any order
  and the one division rounds the same rational: bytes equal the restatement's.
* Kernel alone, Gaussian keys: 2 ml non-negative terms in any order, two roundings per term and the quotient: (2 ml + 8) 2^-53 relative.
* Through wu.swd: the projections of either implementation are off by at most 147 u |d| |dir|, sorting is 1-Lipschitz in the sup norm and
  so is W1 in either column: |w_j - ref_j| <= 4 * 147 * u * R, R the largest descriptor row 2-norm, as tests/test_gpu_swd.py argues.

Outputs live in tests/_gpu_guard.py buffers: NaN before the call, guards on both sides checked after it."""
import functools

import numpy as np
import pytest
import torch

import _swd_cases as CASES
import _swd_ref as R
import _swd_unequal_ref as REF
from _gpu_guard import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53


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


def _abi_unequal(a, b):
    """a (ndirs, m1), b (ndirs, m2) float64 with ascending rows -> (ndirs,) float64 from the kernel; the inputs must come back unchanged."""
    L, _ = _lib()
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    w = GuardedF64(a.shape[0])
    L.call("wu_swd_distance_unequal", ad.data_ptr(), a.shape[1], bd.data_ptr(), b.shape[1], a.shape[0], w.ptr, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(ad.cpu().numpy(), a) and np.array_equal(bd.cpu().numpy(), b), "wu_swd_distance_unequal: input modified"
    return w.numpy("wu_swd_distance_unequal")


def _pair(name):
    b = _block()
    named = {"b-1,b": (b - 1, b), "2b+17,5b+3": (2 * b + 17, 5 * b + 3), "2^21,2^21-1": (1 << 21, (1 << 21) - 1)}
    return named[name] if name in named else tuple(int(v) for v in name.split(","))


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1,2", "2,1", "2,3", "6,4", "63,64", "64,65", "255,256", "256,257", "257,512", "256,512", "1,257",
                                  "1000,7", "b-1,b", "2b+17,5b+3", "70001,65537", "2^21,2^21-1"])
def test_kernel_is_exact_on_integer_keys(name):
    """257 and 256 against 512 keys: ml is past one pass of 256 threads, and in the second pair ms divides ml (w1 is 0 throughout).
    70001 x 65537 is past 2^32.  2^21 against 2^21 - 1: one direction and keys in [0, 100), the integer sum below 2^42 * 100 < 2^53."""
    m1, m2 = _pair(name)
    rng = np.random.RandomState(m1 % 1000 + 7 * (m2 % 1000))
    if max(m1, m2) == 1 << 21:
        a, b = rng.randint(0, 100, (1, m1)), rng.randint(0, 100, (1, m2))
    else:
        a, b = rng.randint(-50, 51, (3, m1)), rng.randint(-50, 51, (3, m2))
    a, b = np.sort(a.astype(np.float64), axis=1), np.sort(b.astype(np.float64), axis=1)
    want = REF.closed_form_rows(a, b)
    got = _abi_unequal(a, b)
    assert want.min() > 0 and np.array_equal(got, want), f"({m1}, {m2}): {got} against {want}"
    assert _abi_unequal(b, a).tobytes() == got.tobytes()                 # W(a, b) and W(b, a): the walk is over the longer column
    assert _abi_unequal(a, b).tobytes() == got.tobytes()                 # two runs


def test_kernel_takes_equal_counts_too():
    rng = np.random.RandomState(2)
    for m in (1, 256, 300):
        a, b = np.sort(rng.randint(-50, 51, (3, m)).astype(np.float64), axis=1), np.sort(rng.randint(-50, 51, (3, m)).astype(np.float64), axis=1)
        assert np.array_equal(_abi_unequal(a, b), np.abs(a - b).sum(axis=1) / m)


@pytest.mark.parametrize("name", ["1000,7", "2b+17,5b+3"])
def test_kernel_within_the_summation_bound_on_gaussian_keys(name):
    m1, m2 = _pair(name)
    rng = np.random.RandomState(m1 % 1000 + m2 % 1000)
    a, b = np.sort(rng.randn(3, m1), axis=1), np.sort(0.8 * rng.randn(3, m2) + 0.1, axis=1)
    want = REF.closed_form_rows(a, b)
    got = _abi_unequal(a, b)
    bound = (2 * max(m1, m2) + 8) * U
    rel = np.abs(got - want) / want
    print(f"({m1}, {m2}): largest relative difference from the float64 restatement {rel.max():.3e}, bound {bound:.3e}")
    assert np.all(rel <= bound)
    assert _abi_unequal(b, a).tobytes() == got.tobytes()


def test_out_of_range_arguments_are_rejected_without_a_launch():
    _, lib = _lib()
    keys = torch.zeros(64, dtype=torch.float64, device=DEV)
    out = GuardedF64(8)
    big = (1 << 21) + 1
    for m1, m2, nd in ((0, 4, 2), (4, 0, 2), (big, 4, 2), (4, big, 2), (4, 5, 0), (4, 5, 4097)):
        assert lib.wu_swd_distance_unequal(keys.data_ptr(), m1, keys.data_ptr(), m2, nd, out.ptr, _stream()) < 0
        assert b"wu_swd_distance_unequal" in lib.wu_last_error()
    assert lib.wu_swd_distance_unequal(None, 4, keys.data_ptr(), 5, 2, out.ptr, _stream()) < 0
    assert lib.wu_swd_distance_unequal(keys.data_ptr(), 4, None, 5, 2, out.ptr, _stream()) < 0
    assert lib.wu_swd_distance_unequal(keys.data_ptr(), 4, keys.data_ptr(), 5, 2, None, _stream()) < 0
    assert b"NULL" in lib.wu_last_error()
    torch.cuda.synchronize()
    out.untouched("wu_swd_distance_unequal")


# ---------------------------------------------------------------------------------------------------------------------------------
# through wu.swd
# ---------------------------------------------------------------------------------------------------------------------------------
def _bound(*descs):
    r = max(np.sqrt(np.square(d.astype(np.float64)).sum(axis=1)).max() for d in descs)
    return 4 * 147 * U * r


@pytest.mark.parametrize("which", ["100,37", "b+1,2b+17"])
def test_sliced_wasserstein_exact(which, monkeypatch):
    from wu import swd
    b = _block()
    m1, m2 = {"100,37": (100, 37), "b+1,2b+17": (b + 1, 2 * b + 17)}[which]
    d1, d2 = CASES.normalised_descriptors(m1, 11), (0.8 * CASES.normalised_descriptors(m2, 12) + 0.1).astype(np.float32)
    dirs = CASES.unit_dirs(70, 13)
    ref = REF.closed_form_rows(R.sorted_projections(d1, dirs), R.sorted_projections(d2, dirs))
    t1, t2 = torch.from_numpy(d1).to(DEV), torch.from_numpy(d2).to(DEV)
    got = swd.sliced_wasserstein(t1, t2, dirs, unequal="exact")
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (70,)
    w = got.cpu().numpy()
    bound = _bound(d1, d2)
    print(f"({m1}, {m2}): |w - ref| max {np.abs(w - ref).max():.3e}, bound {bound:.3e}, w in [{ref.min():.4f}, {ref.max():.4f}]")
    assert ref.min() > 0 and np.all(np.abs(w - ref) <= bound)
    assert swd.sliced_wasserstein(t2, t1, dirs, unequal="exact").cpu().numpy().tobytes() == w.tobytes()
    for chunk in (1, 7):
        assert swd.sliced_wasserstein(t1, t2, dirs, dir_chunk=chunk, unequal="exact").cpu().numpy().tobytes() == w.tobytes()
    monkeypatch.setattr(swd, "PAIR_BYTES", 8 * (m1 + m2) * 16)             # 16 directions per group: 5 groups, the last of 6
    assert swd.sliced_wasserstein(t1, t2, dirs, unequal="exact").cpu().numpy().tobytes() == w.tobytes()
    monkeypatch.undo()
    with pytest.raises(ValueError, match="unequal"):
        swd.sliced_wasserstein(t1, t2, dirs)
    same = swd.sliced_wasserstein(t1, t1 * 0.5, dirs)
    assert swd.sliced_wasserstein(t1, t1 * 0.5, dirs, unequal="exact").cpu().numpy().tobytes() == same.cpu().numpy().tobytes()


@pytest.mark.parametrize("k", [2, 3])
def test_a_set_against_itself_duplicated_is_zero(k):
    """Every key of the longer column k times: x_i owns a k-th of y_(i // k)'s interval, w1 = 0, and x_i == y_(i // k) to the bit (a
    projection depends on its own two rows only)."""
    from wu import swd
    d1 = torch.from_numpy(CASES.normalised_descriptors(100, 5)).to(DEV)
    dirs = CASES.unit_dirs(70, 6)
    w = swd.sliced_wasserstein(d1, d1.repeat(k, 1), dirs, unequal="exact")
    assert torch.equal(w, torch.zeros_like(w))
    w = swd.sliced_wasserstein(d1.repeat(k, 1), d1, dirs, unequal="exact")
    assert torch.equal(w, torch.zeros_like(w))


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
KW = dict(P=8, repeats=2, dirs_per_repeat=8)


@functools.lru_cache(maxsize=None)
def _e2e():
    x, y, z = CASES.images(4, 32, 32, 21), CASES.images(4, 32, 32, 22), CASES.images(6, 32, 32, 24)
    y = (0.7 * y + 0.1 * np.random.RandomState(23).uniform(-1, 1, y.shape)).astype(np.float32)
    return x, y, z, torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(z).to(DEV)


def _bank(images, seed=0, **kw):
    from wu import swd
    return swd.DescriptorBank(seed=seed, **{**KW, **kw}).add(images)


def test_swd_end_to_end_on_unequal_sets():
    from wu import swd
    x, y, _, xd, yd, _ = _e2e()
    r = swd.swd(xd, yd[:3], seed=4, unequal="exact", **KW)
    assert len(r.levels) == 2
    pos, dirs = swd.draw(4, 2, [(32, 32), (16, 16)], 4, 8, 16)
    da, db = R.descriptors(x, pos, 0.5, 0.5, 2), R.descriptors(y[:3], pos[:, :3], 0.5, 0.5, 2)
    for l in range(2):
        na, nb = R.normalize(da[l]), R.normalize(db[l])
        want = REF.closed_form_rows(R.sorted_projections(na, dirs), R.sorted_projections(nb, dirs)).mean()
        bound = _bound(na, nb)
        print(f"level {l}: swd {r.levels[l] / 1e3:.6f} ref {want:.6f} diff {abs(r.levels[l] / 1e3 - want):.3e} bound {bound:.3e}")
        assert want > 1e-3 and abs(r.levels[l] / 1e3 - want) <= bound
    assert r.mean == pytest.approx(np.mean(r.levels), rel=1e-15)
    assert swd.swd(yd[:3], xd, seed=4, unequal="exact", **KW) == r                       # the larger set may come second
    assert swd.swd(xd, yd, seed=4, unequal="exact", **KW) == swd.swd(xd, yd, seed=4, **KW)  # equal counts: the default's values
    with pytest.raises(ValueError, match="image size"):
        swd.swd(xd, yd[:3, :, :16, :16], unequal="exact", **KW)


def test_bank_in_two_batches_equals_one_and_compare():
    from wu import swd
    _, _, _, xd, yd, zd = _e2e()
    whole, parts = _bank(zd), _bank(zd[:4]).add(zd[4:])
    assert whole.count == parts.count == 6
    for a, b in zip(whole.descriptors(), parts.descriptors()):
        assert a.shape == (48, 147) and torch.equal(a, b)
    zero = swd.compare(whole, parts)
    assert zero.levels == (0.0, 0.0) and zero.mean == 0.0
    assert swd.compare(_bank(xd, 4), _bank(yd[:3], 4)) == swd.swd(xd, yd[:3], seed=4, unequal="exact", **KW)
    assert swd.compare(_bank(xd, 4), _bank(yd, 4)) == swd.swd(xd, yd, seed=4, **KW)
    assert swd.compare(whole, _bank(xd), dir_chunk=3) == swd.compare(_bank(xd), whole)
    for other in (_bank(xd, seed=1), _bank(xd, P=4), _bank(xd, repeats=1), _bank(xd, levels=1), _bank(xd[..., :16, :]),
                  swd.DescriptorBank(value_range=(0, 1), **KW).add(xd)):
        with pytest.raises(ValueError, match="must share"):
            swd.compare(whole, other)
    with pytest.raises(ValueError, match="after"):
        whole.add(xd[..., :16, :])


def test_accumulator_with_references_equals_compare_of_the_concatenations():
    from wu import swd
    from wu.evaluate import SlicedWasserstein
    _, _, _, xd, yd, zd = _e2e()
    bank0, bank1 = _bank(zd, 9), _bank(zd[:3], 9)
    want = [swd.compare(_bank(yd, 9), bank0), swd.compare(_bank(xd, 9), bank1)]
    acc = SlicedWasserstein(seed=9, reference=[bank0, bank1], **KW)
    acc.update(xd[:3], torch.stack([yd[:3], xd[:3]]))
    acc.update(xd[3:], torch.stack([yd[3:], xd[3:]]))
    assert acc.real == [] and acc.compute() == want
    shared = SlicedWasserstein(seed=9, reference=bank0, **KW)                               # one bank for every row: sorted once per group
    shared.update(xd, torch.stack([yd, xd]))
    assert shared.compute() == [want[0], swd.compare(_bank(xd, 9), bank0)]
    plain = SlicedWasserstein(seed=9, reference=bank1, **KW)
    plain.update(xd[:1], yd[:1])
    plain.update(xd[1:], yd[1:])
    assert plain.compute() == swd.compare(_bank(yd, 9), bank1)
    with pytest.raises(ValueError, match="must share"):
        wrong = SlicedWasserstein(seed=8, reference=bank0, **KW)
        wrong.update(xd, yd)
        wrong.compute()
    with pytest.raises(ValueError, match="reference banks"):
        short = SlicedWasserstein(seed=9, reference=[bank0], **KW)
        short.update(xd, torch.stack([yd, xd]))
        short.compute()


class _Sweep:
    """A stand-in generator: row r of the sweep is the batch scaled by a class-dependent gain."""

    def sweep(self, batch, rows, max_images):
        gains = 1.0 - 0.1 * torch.arange(rows.shape[0], device=batch.device, dtype=batch.dtype)
        return batch.unsqueeze(0) * gains.view(-1, 1, 1, 1, 1)


def _classifier(images):
    return torch.stack([images.mean((1, 2, 3)), images.amax((1, 2, 3)), images.amin((1, 2, 3))], 1)


def test_class_transfer_evaluation_takes_an_accumulator_with_references():
    from wu import swd
    from wu.evaluate import ClassTransferEval, SlicedWasserstein
    _, _, _, xd, _, zd = _e2e()
    banks = [_bank(zd), _bank(zd[:5]), _bank(xd)]
    acc = SlicedWasserstein(reference=banks, **KW)
    plain, with_swd = ClassTransferEval(_Sweep(), _classifier, 3), ClassTransferEval(_Sweep(), _classifier, 3, swd=acc)
    for ev in (plain, with_swd):
        ev.update(xd[:2])
        ev.update(xd[2:])
    assert torch.equal(plain.confusion(), with_swd.confusion()) and plain.report() == with_swd.report()
    per_class = acc.compute()
    assert len(per_class) == 3 and per_class[0] == swd.compare(_bank(xd), banks[0]) and per_class[0].mean > 0
    fakes = _Sweep().sweep(xd, torch.eye(3, device=DEV), 0)
    assert per_class[1] == swd.compare(_bank(fakes[1]), banks[1]) and per_class[2] == swd.compare(_bank(fakes[2]), banks[2])


def test_command_line_exact(tmp_path, capsys):
    from PIL import Image
    from wu import swd
    a, b = CASES.images_u8(5, 32, 32, 31), CASES.images_u8(7, 32, 32, 32)
    for name, arr in (("a", a), ("b", b)):
        (tmp_path / name).mkdir()
        for i, img in enumerate(arr):
            Image.fromarray(img.transpose(1, 2, 0)).save(tmp_path / name / f"{i:02d}.png")
    args = [str(tmp_path / "a"), str(tmp_path / "b"), "--patches", "8", "--repeats", "2", "--dirs", "8", "--seed", "3"]
    assert swd.main(args + ["--unequal", "exact"]) == 0
    out = capsys.readouterr().out
    assert "images: 5 against 7" in out and "random subset" not in out and "images per set" not in out
    want = swd.swd(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), seed=3, value_range="uint8", unequal="exact", **KW)
    lines = [ln for ln in out.splitlines() if ln.startswith("SWD")]
    assert lines == [f"SWD x 1e3, level {l}: {v:.4f}" for l, v in enumerate(want.levels)] + [f"SWD x 1e3, mean: {want.mean:.4f}"]
    assert swd.main(args + ["--unequal", "subset"]) == 0
    explicit = capsys.readouterr().out
    assert swd.main(args) == 0
    assert capsys.readouterr().out == explicit and "random subset" in explicit and "images per set: 5" in explicit
    bank = swd.DescriptorBank.from_dir(str(tmp_path / "b"), seed=3, **KW)
    assert bank.count == 7 and bank.value_range == "uint8" and bank.shape == (32, 32)
