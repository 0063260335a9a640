"""The rank-aware Frechet distance on the GPU (csrc/frechet.hip through the C ABI and through wu.frechet) against tests/_frechet_ref.py.

Stages 1 - 3, exact: integer features in {0..3} make every inner product and every row / column / total sum an exact integer whatever the
order, so the centred matrix must EQUAL the restatement's bytes (the four centring terms in the stated order, one rounding each), and so
must mu, |x_i - mu|^2 and s (the restatement adds in the kernels' order).  Jacobi stage: singular values against np.linalg.svd within
K_GPU (m + n) 2^-53 sigma_1 each (K_GPU = 8 x the restatement's own recorded worst ratio against LAPACK, tests/test_frechet_cpu.py).  End
to end: within _frechet_ref.bound of the restatement (derived there, not tuned)."""
import functools

import numpy as np
import pytest
import torch

import _frechet_ref as R
from _padded_rows import padded as _padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

EXACT_SHAPES = [(2, 2, 1), (2, 3, 5), (63, 65, 7), (64, 64, 64), (65, 129, 100), (129, 63, 33)]


@functools.lru_cache(maxsize=None)
def _exact(shape):
    n1, n2, D = shape
    rng = np.random.RandomState(1000 * n1 + 10 * n2 + D)
    x = rng.randint(0, 4, (n1, D)).astype(np.float32)
    y = rng.randint(0, 4, (n2, D)).astype(np.float32)
    x[0, 0], y[-1, -1] = 3.0, 1.0                       # never all-equal, never symmetric: V differs from its transpose
    y[0, 0] = 0.0
    return x, y, R.centred_cross_gram(x, y), R.moments(x), R.moments(y)


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), \
        f"{what}: not bit-identical; max |diff| {np.nanmax(np.abs(got - want))}, got {got.reshape(-1)[:3]}, want {want.reshape(-1)[:3]}"


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "n%dx%d_D%d" % s)
def test_centred_cross_gram_exact_c_abi(shape):
    """wu_fd_cross_gram on contiguous uploads into a NaN-filled workspace: the matrix equals the restatement's, and the padding columns
    between nl and ld stay untouched."""
    from wu import _lib
    lib = _lib.load()
    n1, n2, D = shape
    x, y, want, _, _ = _exact(shape)
    ns, nl = min(n1, n2), max(n1, n2)
    ld, nbytes = lib.wu_fd_ld(n1, n2), lib.wu_fd_workspace_bytes(n1, n2, D)
    assert ld >= nl and nbytes == (ns * ld + ns + nl + 1) * 8
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    ws = torch.full((nbytes // 8,), NAN, dtype=torch.float64, device=DEV)
    _lib.call("wu_fd_cross_gram", xd.data_ptr(), D, n1, yd.data_ptr(), D, n2, D, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    full = ws[:ns * ld].view(ns, ld).cpu().numpy()
    assert want.shape == (ns, nl)
    _same_bytes(full[:, :nl], want, "centred matrix")
    assert np.isnan(full[:, nl:]).all()
    # the sums behind it are exact integers
    g = R.cross_gram(x, y)
    tail = ws[ns * ld:].cpu().numpy()
    _same_bytes(tail[:ns], g.sum(axis=1), "row sums")
    _same_bytes(tail[ns:ns + nl], g.sum(axis=0), "column sums")
    assert tail[ns + nl] == g.sum()


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "n%dx%d_D%d" % s)
def test_centred_cross_gram_and_moments_exact_strided_and_poisoned(shape):
    """Through wu.frechet on views of wider and longer buffers: ld > D with NaN padding columns, NaN rows after n1 / n2."""
    from wu import frechet
    n1, n2, D = shape
    x, y, want, mx, my = _exact(shape)
    f1, f2 = _padded(x, D + 3, 2), _padded(y, D + 5, 1)
    assert f1.stride(0) == D + 3 and f2.stride(0) == D + 5
    v, _ws = frechet.centred_cross_gram(f1, f2)
    assert v.dtype == torch.float64 and tuple(v.shape) == want.shape
    _same_bytes(v.cpu().numpy(), want, "centred matrix")
    for f, (mu, dev2, s), name in ((f1, mx, "set 1"), (f2, my, "set 2")):
        gmu, gdev2, gs = frechet.moments(f)
        _same_bytes(gmu.cpu().numpy(), mu, f"mu of {name}")
        _same_bytes(gdev2.cpu().numpy(), dev2, f"dev2 of {name}")
        assert gs.item() == s, f"s of {name}: {gs.item()} != {s}"


# ---- the Jacobi stage ---------------------------------------------------------------------------------------------------------------------------
CASES = R.jacobi_cases()


@functools.lru_cache(maxsize=None)
def _device_svd(name):
    from wu import frechet
    m = torch.from_numpy(CASES[name]).to(DEV)
    before = m.clone()
    sigma, total, rotations = frechet.singular_values(m, info=True)
    assert torch.equal(m, before)                                              # the input is not modified
    return sigma.cpu().numpy(), float(total.item()), rotations


@pytest.mark.parametrize("name", sorted(CASES))
def test_singular_values_against_lapack(name):
    M = CASES[name]
    sigma, total, rotations = _device_svd(name)
    assert sigma.shape == (M.shape[0],) and rotations[-1] == 0 and all(r > 0 for r in rotations[:-1])
    sv = np.linalg.svd(M, compute_uv=False)
    want = np.zeros(M.shape[0])
    want[:len(sv)] = sv
    tol = R.sv_tolerance(M.shape, sv[0], R.K_GPU)
    err = np.abs(np.sort(sigma)[::-1] - want).max()
    print(f"{name}: {len(rotations)} sweeps, rotations {rotations}, max |sigma - svd| {err:.3g}, tolerance {tol:.3g}")
    assert np.isfinite(sigma).all() and err <= tol
    acc = 0.0
    for v in sigma:
        acc += v
    assert total == acc                                                        # the sum in index order


def test_singular_values_special_cases():
    sigma, total, rotations = _device_svd("zero_5x9")
    assert rotations == [0] and np.array_equal(sigma, np.zeros(5)) and total == 0.0       # one sweep, no rotation, no NaN
    sigma, _, rotations = _device_svd("hadamard_16x16")
    assert rotations == [0]
    _same_bytes(sigma, R.HADAMARD_SIGMA, "norms of orthogonal integer rows")
    sigma, _, _ = _device_svd("130x70")
    assert (sigma == 0.0).sum() >= 60                                          # more vectors than length: the surplus ends at zero
    assert _device_svd("1x5")[2] == [0]
    sigma, _, rotations = _device_svd("twin_rows_6x10")                        # zeta = 0 in the first rotation of the twins
    assert rotations[0] > 0 and np.isfinite(sigma).all()


def test_register_and_reread_paths_agree_with_the_restatement():
    """4 x 2048 keeps the pair in registers, 4 x 2049 reads it again; both add in the restatement's order."""
    for name in ("4x2048", "4x2049"):
        sigma, _, rotations = _device_svd(name)
        want, _, want_rot = R.singular_values(CASES[name])
        print(f"{name}: rotations {rotations}, restatement {want_rot}, max |sigma - restatement| {np.abs(sigma - want).max():.3g}")
        assert np.abs(sigma - want).max() <= R.sv_tolerance(CASES[name].shape, want.max(), R.K_GPU)


def test_max_sweeps_raises():
    from wu import frechet
    m = torch.from_numpy(CASES["64x64"]).to(DEV)
    with pytest.raises(RuntimeError, match="rotations in sweep 1"):
        frechet.singular_values(m, max_sweeps=1)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
TERMS = ("fid", "trace_sqrt", "mean_term", "trace1", "trace2")


@functools.lru_cache(maxsize=None)
def _real(shape):
    n1, n2, D = shape
    rng = np.random.RandomState(n1 + n2 + D)
    x = rng.rand(n1, D).astype(np.float32)
    y = (1.2 * rng.rand(n2, D) ** 2).astype(np.float32)
    ref = R.frechet_distance(x, y)
    return x, y, ref, R.bound(x, y, ref, R.K_GPU)


@functools.lru_cache(maxsize=None)
def _device_fd(shape, swapped=False):
    from wu import frechet
    x, y, _, _ = _real(shape)
    a, b = _padded(x, x.shape[1] + 8, 1), _padded(y, y.shape[1], 2)
    return frechet.frechet_distance(b, a) if swapped else frechet.frechet_distance(a, b)


@pytest.mark.parametrize("shape", [(96, 80, 2048), (70, 200, 64)], ids=lambda s: "n%dx%d_D%d" % s)
def test_frechet_distance_within_the_derived_bound(shape):
    """Every term within _frechet_ref.bound of the restatement: ns times the singular-value tolerance of both sides, the nuclear norm of the
    two Gram matrices' rounding difference (per entry (D + 4) 2^-53 sum_k |x_ik| |y_jk| and the centring terms' sums), and the moments'
    (D + n) 2^-53 sums -- derived in bound's docstring.  Swapping the sets moves fid by no more than that either."""
    x, y, ref, bound = _real(shape)
    got = _device_fd(shape)
    for k in TERMS:
        err = abs(getattr(got, k) - ref[k])
        print(f"{shape} {k}: {getattr(got, k)!r} ref {ref[k]!r} |diff| {err:.3g} bound {bound[k]:.3g}")
        assert err <= bound[k], f"{k}: |{getattr(got, k)} - {ref[k]}| = {err} over the bound {bound[k]}"
    print(f"{shape}: {got.sweeps} sweeps (restatement {ref['sweeps']}), rotations {got.rotations}")
    assert got.sweeps == len(got.rotations) and got.rotations[-1] == 0
    assert got.singular_values.shape == (min(shape[:2]),) and got.singular_values.dtype == torch.float64 and got.singular_values.is_cuda
    assert got.fid > 1.0                                                       # the two sets do differ
    back = _device_fd(shape, True)
    assert abs(back.fid - got.fid) <= bound["fid"]
    assert abs(back.trace1 - got.trace2) <= bound["trace2"] and abs(back.trace_sqrt - got.trace_sqrt) <= bound["trace_sqrt"]


def test_two_runs_give_identical_bytes():
    from wu import frechet
    x, y, _, _ = _real((96, 80, 2048))
    runs = []
    for _ in range(2):
        a, b = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
        v, _ws = frechet.centred_cross_gram(a, b)
        r = frechet.frechet_distance(a, b)
        runs.append((v.cpu().numpy().tobytes(), r.singular_values.cpu().numpy().tobytes(), np.float64(r.fid).tobytes(), r.rotations))
    assert runs[0] == runs[1]


def test_wrapper_value_errors():
    from wu import frechet
    ok = torch.rand(4, 8, device=DEV)
    with pytest.raises(ValueError, match="float32 CUDA"):
        frechet.frechet_distance(ok.cpu(), ok)
    with pytest.raises(ValueError, match="float32 CUDA"):
        frechet.frechet_distance(ok, ok.double())
    with pytest.raises(ValueError, match="at least 2 rows"):
        frechet.frechet_distance(ok[:1], ok)
    with pytest.raises(ValueError, match="widths"):
        frechet.frechet_distance(ok, ok[:, :7])
    big = torch.zeros(1, 8, device=DEV).expand(4097, 8)                        # a shape, not an allocation
    with pytest.raises(ValueError, match="calculate_frechet_distance"):
        frechet.frechet_distance(big, big)
    with pytest.raises(ValueError, match="float64 CUDA"):
        frechet.singular_values(ok)
    with pytest.raises(ValueError, match="outside"):
        frechet.singular_values(torch.zeros(1, 8, dtype=torch.float64, device=DEV).expand(4097, 8))
    with pytest.raises(ValueError, match="max_sweeps"):
        frechet.singular_values(ok.double(), max_sweeps=0)


def test_cli_prints_fid_rows_after_fid_from_feature_npz(tmp_path, capsys):
    """`python -m wu.fid A.npz B.npz --fid-rows`: the new line follows `FID:`; without the flag the output is what it was; a .npz without
    `features` gives the error --kid gives."""
    from wu import fid, frechet
    D = 8
    rng = np.random.RandomState(12)
    x, y = rng.rand(40, D).astype(np.float32), (0.8 * rng.rand(33, D)).astype(np.float32)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    xd = x.astype(np.float64)
    np.savez(pa, features=x, mu=xd.mean(axis=0), sigma=np.cov(xd, rowvar=False))
    yd = y.astype(np.float64)
    np.savez(pb, features=y, mu=yd.mean(axis=0), sigma=np.cov(yd, rowvar=False))       # without --fid-rows a .npz is read for mu / sigma
    base = [pa, pb, "--weights", "unused.pth"]
    assert fid.main(base) == 0
    plain = capsys.readouterr().out
    assert len(plain.strip().splitlines()) == 1 and plain.startswith("FID: ")
    assert fid.main(base + ["--fid-rows"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0] + "\n" == plain and lines[1].startswith("FID (rows): ") and lines[1].endswith(" sweeps)")
    r = frechet.frechet_distance(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    assert lines[1] == f"FID (rows): {r.fid} ({r.sweeps} sweeps)"
    ref = R.frechet_distance(x, y)
    assert abs(r.fid - ref["fid"]) <= R.bound(x, y, ref, R.K_GPU)["fid"]
    # n >> D: scipy is trustworthy here and the two lines agree
    assert abs(r.fid - float(lines[0][5:])) <= 1e-9 * max(1.0, abs(r.fid))
    assert fid.main(base + ["--fid-rows", "--kid", "--kid-subsets", "2", "--kid-subset-size", "20"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["FID", "FID (rows)", "KID"]
    np.savez(str(tmp_path / "c.npz"), mu=np.zeros(D), sigma=np.eye(D))
    errors = []
    for flag in ("--fid-rows", "--kid"):
        with pytest.raises(ValueError, match="features") as e:
            fid.main([pa, str(tmp_path / "c.npz"), "--weights", "unused.pth", flag])
        errors.append(str(e.value))
    assert errors[0] == errors[1]
