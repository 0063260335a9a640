"""csrc/adain_style.hip (wu_adain_style_{fwd,bwd} and _multi) against the oracles of tests/_style_ref.py: integer data for which y4,
y_mean, dW and db are exact in any summation order (bit equality; y_std within 4 ulp), and Gaussian data through wu.functional against
float64 autograd with running error bounds.  The derivations are in the docstring of _style_ref; tests/test_style_ref_cpu.py shows that
the checks reject a dropped sample lane, a wrong row index, a dropped input feature and a missing bias.

Shapes: N in {1, 7, 8, 9, 19} (the eight sample lanes of the backward: idle lanes, exactly one sample each, a ragged second and third
lap of the stride-8 walk), C in {1, 3, 8, 40, 65} (odd C leaves a partly valid wave at the end of a level, 65 needs a third workgroup),
nc in {1, 5, 31, 32} (32 fills the register array).  Outputs live in NaN-filled buffers with guard floats on both sides; inputs are
compared with their host copies after every call."""
import ctypes

import numpy as np
import pytest
import torch

import _style_ref as R
from _gpu_guard import Guarded, Input, _dev, _I, _lib, _P, _stream

pytestmark = pytest.mark.gpu

# (N, C, nc): every value of each set appears; N = 19 pairs with C = 65 and nc = 32
SHAPES = [(1, 1, 1), (7, 3, 5), (8, 8, 31), (9, 40, 5), (19, 65, 32), (8, 3, 32), (9, 65, 1)]
# _multi: 1 to 4 levels, the largest level never first (but for one level), an odd C and a level with C = 1 wherever there is room
LEVELS = {1: (7, 1, [40]), 2: (8, 31, [3, 65]), 3: (9, 5, [8, 65, 1]), 4: (19, 32, [3, 40, 1, 65])}          # levels -> (N, nc, [C])
EPS = [1e-5, 1e-3, 0.25, 1e-8]


def _F(vals):
    return (ctypes.c_float * len(vals))(*vals)


class Fwd:
    def __init__(self, c, y, with_y4=True):
        self.c, self.y = c, y
        self.w = Input(c["w"])
        self.b = Input(c["b"]) if c["b"] is not None else None
        n = c["N"] * c["C"]
        self.y_std, self.y_mean = Guarded(n), Guarded(n)
        self.y4 = Guarded(4 * n) if with_y4 else None

    def check(self, what):
        c = self.c
        self.y.unchanged(f"{what}: y")
        self.w.unchanged(f"{what}: w")
        if self.b is not None:
            self.b.unchanged(f"{what}: b")
        shape = (c["N"], c["C"])
        R.check_fwd(c, dict(y_std=self.y_std.numpy(f"{what}: y_std", shape), y_mean=self.y_mean.numpy(f"{what}: y_mean", shape),
                            y4=self.y4.numpy(f"{what}: y4", shape + (4,)) if self.y4 is not None else None), what)


class Bwd:
    def __init__(self, c, y, accumulate, with_db=True):
        self.c, self.y, self.accumulate = c, y, accumulate
        self.inputs = {k: Input(c[k]) for k in ("d_std", "d_mean", "y4", "y_std", "y_mean")}
        self.dw = Guarded(4 * c["C"] * c["nc"], c["dw0"] if accumulate else None)
        self.db = Guarded(4 * c["C"], c["db0"] if accumulate else None) if with_db else None

    def check(self, what):
        c = self.c
        self.y.unchanged(f"{what}: y")
        for k, t in self.inputs.items():
            t.unchanged(f"{what}: {k}")
        R.check_bwd(c, self.dw.numpy(f"{what}: dW", (4 * c["C"], c["nc"])), self.db.numpy(f"{what}: db") if self.db is not None else None,
                    self.accumulate, what)


def _opt(x):
    return x.ptr if x is not None else None


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_forward_exact(N, C, nc, bias):
    c = R.fwd_case(N, C, nc, 3, bias)
    y = Input(c["y"])
    for with_y4 in (True, False):
        f = Fwd(c, y, with_y4)
        _lib().call("wu_adain_style_fwd", y.ptr, f.w.ptr, _opt(f.b), float(c["eps"]), f.y_std.ptr, f.y_mean.ptr, _opt(f.y4), N, C, nc, _stream())
        torch.cuda.synchronize()
        f.check(f"single y4 {with_y4}")


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("tier", ["a", "b"])
def test_backward_exact(N, C, nc, tier):
    """accumulate = 0 into NaN-filled dW / db, accumulate = 1 on top of integers, and db = NULL (a layer without bias)."""
    c = R.bwd_case(N, C, nc, 5, tier)
    y = Input(c["y"])
    for accumulate, with_db in ((0, True), (1, True), (0, False), (1, False)):
        b = Bwd(c, y, accumulate, with_db)
        i = b.inputs
        _lib().call("wu_adain_style_bwd", i["d_std"].ptr, i["d_mean"].ptr, y.ptr, i["y4"].ptr, i["y_std"].ptr, i["y_mean"].ptr, b.dw.ptr, _opt(b.db),
                    N, C, nc, accumulate, _stream())
        torch.cuda.synchronize()
        b.check(f"single db {with_db}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_forward_multi_exact(levels):
    N, nc, Cs = LEVELS[levels]
    assert levels == 1 or Cs[0] != max(Cs)
    yi = R.int_y(N, nc, 70)
    y = Input(yi)
    cases = [R.fwd_case(N, C, nc, 80 + i, bias=(i != 1), eps=EPS[i], y=yi) for i, C in enumerate(Cs)]
    fs = [Fwd(c, y, with_y4=(i != 2)) for i, c in enumerate(cases)]
    _lib().call("wu_adain_style_fwd_multi", levels, y.ptr, _P([f.w.ptr for f in fs]), _P([_opt(f.b) for f in fs]), _F([c["eps"] for c in cases]),
                _P([f.y_std.ptr for f in fs]), _P([f.y_mean.ptr for f in fs]), _P([_opt(f.y4) for f in fs]), N, _I(Cs), nc, _stream())
    torch.cuda.synchronize()
    for i, f in enumerate(fs):
        f.check(f"multi level {i} of {levels}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_backward_multi_exact(levels, accumulate):
    N, nc, Cs = LEVELS[levels]
    yi = R.int_y(N, nc, 71)
    y = Input(yi)
    cases = [R.bwd_case(N, C, nc, 90 + i, "ab"[i % 2], y=yi) for i, C in enumerate(Cs)]
    bs = [Bwd(c, y, accumulate, with_db=(i != 1)) for i, c in enumerate(cases)]
    col = lambda k: _P([b.inputs[k].ptr for b in bs])  # noqa: E731
    _lib().call("wu_adain_style_bwd_multi", levels, col("d_std"), col("d_mean"), y.ptr, col("y4"), col("y_std"), col("y_mean"),
                _P([b.dw.ptr for b in bs]), _P([_opt(b.db) for b in bs]), N, _I(Cs), nc, accumulate, _stream())
    torch.cuda.synchronize()
    for i, b in enumerate(bs):
        b.check(f"multi level {i} of {levels}")


def test_rejections_write_nothing():
    """nc = 33, levels = 5 and a y4 that is not 16-byte aligned: RuntimeError, no output touched."""
    lib = _lib()
    N, C = 7, 3
    wide = R.fwd_case(N, C, 32, 3)
    y33 = Input(np.ones((N, 33), dtype=np.float32))
    w33 = Input(np.ones((4 * C, 33), dtype=np.float32))
    f = Fwd(wide, y33)
    with pytest.raises(RuntimeError):
        lib.call("wu_adain_style_fwd", y33.ptr, w33.ptr, f.b.ptr, 1e-5, f.y_std.ptr, f.y_mean.ptr, f.y4.ptr, N, C, 33, _stream())
    with pytest.raises(RuntimeError):
        lib.call("wu_adain_style_fwd_multi", 1, y33.ptr, _P([w33.ptr]), _P([f.b.ptr]), _F([1e-5]), _P([f.y_std.ptr]), _P([f.y_mean.ptr]),
                 _P([f.y4.ptr]), N, _I([C]), 33, _stream())
    c = R.fwd_case(N, C, 5, 3)
    y = Input(c["y"])
    with pytest.raises(RuntimeError):         # misaligned y4: one float into its buffer
        lib.call("wu_adain_style_fwd", y.ptr, f.w.ptr, f.b.ptr, 1e-5, f.y_std.ptr, f.y_mean.ptr, f.y4.ptr + 4, N, C, 5, _stream())
    with pytest.raises(RuntimeError):
        lib.call("wu_adain_style_fwd_multi", 1, y.ptr, _P([f.w.ptr]), _P([f.b.ptr]), _F([1e-5]), _P([f.y_std.ptr]), _P([f.y_mean.ptr]),
                 _P([f.y4.ptr + 4]), N, _I([C]), 5, _stream())
    fs = [Fwd(c, y) for _ in range(5)]
    with pytest.raises(RuntimeError):
        lib.call("wu_adain_style_fwd_multi", 5, y.ptr, _P([g.w.ptr for g in fs]), _P([g.b.ptr for g in fs]), _F([1e-5] * 5),
                 _P([g.y_std.ptr for g in fs]), _P([g.y_mean.ptr for g in fs]), _P([g.y4.ptr for g in fs]), N, _I([C] * 5), 5, _stream())
    cb = R.bwd_case(N, C, 5, 5, "b")
    bs = [Bwd(cb, y, 0) for _ in range(5)]
    col = lambda k: _P([b.inputs[k].ptr for b in bs])  # noqa: E731
    with pytest.raises(RuntimeError):
        lib.call("wu_adain_style_bwd_multi", 5, col("d_std"), col("d_mean"), y.ptr, col("y4"), col("y_std"), col("y_mean"),
                 _P([b.dw.ptr for b in bs]), _P([b.db.ptr for b in bs]), N, _I([C] * 5), 5, 0, _stream())
    b, i = bs[0], bs[0].inputs
    with pytest.raises(RuntimeError):
        lib.call("wu_adain_style_bwd", i["d_std"].ptr, i["d_mean"].ptr, y33.ptr, i["y4"].ptr, i["y_std"].ptr, i["y_mean"].ptr, b.dw.ptr, b.db.ptr,
                 N, C, 33, 0, _stream())
    torch.cuda.synchronize()
    for g in [f] + fs:
        for key in ("y_std", "y_mean", "y4"):
            getattr(g, key).untouched(f"forward rejection: {key}")
    for b in bs:
        b.dw.untouched("backward rejection: dW")
        b.db.untouched("backward rejection: db")


# ---------------------------------------------------------------------------------------------------------------------------------
# tolerance tier: wu.functional against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _gauss(N, C, nc, seed, bias, y=None):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)           # noqa: E731
    return dict(y=f(N, nc) if y is None else y, w=f(4 * C, nc) * np.float32(0.3), b=f(4 * C) if bias else None, d_std=f(N, C), d_mean=f(N, C))


def _check_level(what, d, eps, std, mean, w, b):
    ref = R.autograd64(d["y"], d["w"], d["b"], eps, d["d_std"], d["d_mean"])
    bounds = R.tolerance_bounds(d["y"], d["w"], d["b"], eps, d["d_std"], d["d_mean"])
    got = dict(y_std=std.detach().cpu().numpy(), y_mean=mean.detach().cpu().numpy(), dw=w.grad.cpu().numpy(),
               db=b.grad.cpu().numpy() if b is not None else None)
    return R.check_tolerance(what, ref, bounds, got)


@pytest.mark.parametrize("N,C,nc", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_functional_inside_the_running_error_bound(N, C, nc, bias):
    from wu import functional as WF
    dev = _dev()
    d = _gauss(N, C, nc, 2, bias)
    t = {k: torch.from_numpy(v).to(dev) if v is not None else None for k, v in d.items()}
    w = t["w"].requires_grad_(True)
    b = t["b"].requires_grad_(True) if bias else None
    std, mean = WF.adain_style(t["y"], w, b, 1e-5)
    torch.autograd.backward([std, mean], [t["d_std"], t["d_mean"]])
    torch.cuda.synchronize()
    _check_level(f"N{N} C{C} nc{nc} bias {bias}", d, 1e-5, std, mean, w, b)


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_functional_multi_inside_the_running_error_bound(levels):
    from wu import functional as WF
    dev = _dev()
    N, nc, Cs = LEVELS[levels]
    y = np.random.default_rng(6).standard_normal((N, nc)).astype(np.float32)
    ds = [_gauss(N, C, nc, 10 + i, bias=(i != 1), y=y) for i, C in enumerate(Cs)]
    yt = torch.from_numpy(y).to(dev)
    layers, outs_grads = [], []
    for i, d in enumerate(ds):
        w = torch.from_numpy(d["w"]).to(dev).requires_grad_(True)
        b = torch.from_numpy(d["b"]).to(dev).requires_grad_(True) if d["b"] is not None else None
        layers.append((w, b, EPS[i]))
        outs_grads.extend((torch.from_numpy(d["d_std"]).to(dev), torch.from_numpy(d["d_mean"]).to(dev)))
    out = WF.adain_style_multi(yt, layers)
    torch.autograd.backward([t for pair in out for t in pair], outs_grads)
    torch.cuda.synchronize()
    for i, (d, (std, mean), (w, b, eps)) in enumerate(zip(ds, out, layers)):
        _check_level(f"multi level {i} of {levels} (C {Cs[i]})", d, eps, std, mean, w, b)
