"""csrc/spectral_norm.hip (wu_spectral_norm_{fwd,bwd} and _multi) against the oracles of tests/_sn_ref.py: an EXACT tier (integer /
dyadic data: bit equality wherever no sqrt, division or positive non-dyadic sum intervenes, a derived bound behind those) and a
tolerance tier (Gaussian data through wu.functional against stock torch.nn.utils.spectral_norm in float64, running error bounds).
The derivations are in the docstring of _sn_ref; tests/test_sn_ref_cpu.py shows that the checks used here reject the faults they are for.

Every output lives in a NaN-filled buffer with guard floats on both sides, the scratch area is NaN-filled (a read of a slot nobody
wrote poisons the result) with guards after wu_spectral_norm_scratch_floats(), inputs are compared with their host copies afterwards.

Shapes (rows x cols):  (1,5) (1,512) (3,27) (2,6): tails of the 4-way unroll, SNDisc's linear heads and image conv;  (31,255) (32,256)
(33,257): the 32-row group and 256-column block edges;  (64,27) (70,600): interior;  (257,40) (260,300): > 256 rows, sn_finish strides;
(129,1153): five column blocks;  (257,1025): > 262 144 elements, the scale kernel's 1024-block cap laps;  (513,1025): > 524 288 elements,
the backward's 2048-block cap and the dot's kPartMax cap lap.  (4,1) and (9,3) have no room for the reserved columns of the
power-iteration construction: power_iter = 0 and tolerance tiers only."""
import numpy as np
import pytest
import torch

import _sn_ref as R
from _gpu_guard import Guarded, Input, _dev, _I, _lib, _P, _stream

pytestmark = pytest.mark.gpu


def _scratch(rows, cols):
    return Guarded(int(_lib().load().wu_spectral_norm_scratch_floats(rows, cols)))


class Entry:
    """The device side of one weight of a forward call."""

    def __init__(self, W, u, v, w_eff=True, u_save=False, v_save=False):
        self.rows, self.cols = W.shape
        self.W = Input(W)
        self.u, self.v = Guarded(self.rows, u), Guarded(self.cols, v)
        self.sigma = Guarded(2)
        self.w_eff = Guarded(self.rows * self.cols) if w_eff else None
        self.u_save = Guarded(self.rows) if u_save else None
        self.v_save = Guarded(self.cols) if v_save else None
        self.scratch = _scratch(self.rows, self.cols)

    def results(self, power_iter, what):
        self.W.unchanged(what)
        s = self.scratch.numpy(f"{what}: scratch")
        got = dict(u=self.u.numpy(f"{what}: u"), v=self.v.numpy(f"{what}: v"), sigma=self.sigma.numpy(f"{what}: sigma"),
                   u_raw=s[self.cols:self.cols + self.rows])               # scratch layout: [W^T u (cols) | W v (rows) | partials ...]
        if power_iter:
            got["v_raw"] = s[:self.cols]
        for key in ("u_save", "v_save"):
            g = getattr(self, key)
            got[key] = g.numpy(f"{what}: {key}") if g is not None else None
        got["w_eff"] = self.w_eff.numpy(f"{what}: w_eff", (self.rows, self.cols)) if self.w_eff is not None else None
        return got


def _fwd_single(e, power_iter, eps):
    _lib().call("wu_spectral_norm_fwd", e.W.ptr, e.rows, e.cols, e.u.ptr, e.v.ptr, int(power_iter), float(eps), e.sigma.ptr,
                e.w_eff.ptr if e.w_eff is not None else None, e.scratch.ptr, _stream())
    torch.cuda.synchronize()


def _fwd_multi(es, power_iter, eps, save_arrays=True):
    opt = lambda key: _P([getattr(e, key).ptr if getattr(e, key) is not None else None for e in es])  # noqa: E731
    _lib().call("wu_spectral_norm_fwd_multi", len(es), _P([e.W.ptr for e in es]), _I([e.rows for e in es]), _I([e.cols for e in es]),
                _P([e.u.ptr for e in es]), _P([e.v.ptr for e in es]), int(power_iter), float(eps), _P([e.sigma.ptr for e in es]),
                opt("w_eff") if any(e.w_eff is not None for e in es) else None, _P([e.scratch.ptr for e in es]),
                opt("u_save") if save_arrays else None, opt("v_save") if save_arrays else None, _stream())
    torch.cuda.synchronize()


class BwdEntry:
    def __init__(self, c):
        self.c = c
        self.rows, self.cols = c["rows"], c["cols"]
        self.inputs = {k: Input(c[k]) for k in ("G", "W", "u", "v", "sigma")}
        self.dw = Guarded(self.rows * self.cols)
        self.scratch = _scratch(self.rows, self.cols)

    def check(self, what):
        for k, t in self.inputs.items():
            t.unchanged(f"{what}: {k}")
        self.scratch.numpy(f"{what}: scratch")
        R.check_bwd(self.c, self.dw.numpy(f"{what}: dw", (self.rows, self.cols)), what)


def _bwd_single(b):
    i = b.inputs
    _lib().call("wu_spectral_norm_bwd", i["G"].ptr, i["W"].ptr, i["u"].ptr, i["v"].ptr, i["sigma"].ptr, b.dw.ptr, b.rows, b.cols,
                b.scratch.ptr, _stream())
    torch.cuda.synchronize()


def _bwd_multi(bs):
    col = lambda k: _P([b.inputs[k].ptr for b in bs])  # noqa: E731
    _lib().call("wu_spectral_norm_bwd_multi", len(bs), col("G"), col("W"), col("u"), col("v"), col("sigma"), _P([b.dw.ptr for b in bs]),
                _I([b.rows for b in bs]), _I([b.cols for b in bs]), _P([b.scratch.ptr for b in bs]), _stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# single-weight calls, exact tier
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", R.POWER_SHAPES)
def test_forward_power_iteration_exact(rows, cols):
    c = R.power_case(rows, cols, 7)
    e = Entry(c["W"], c["u"], c["v0"], w_eff=(rows, cols) != (33, 257))          # one shape without W_eff (NULL)
    _fwd_single(e, 1, c["eps"])
    R.check_power(c, e.results(1, "single"), "single")


@pytest.mark.parametrize("rows,cols", R.POWER_SHAPES + R.NARROW_SHAPES)
def test_forward_without_power_iteration_exact(rows, cols):
    c = R.iter0_case(rows, cols, 3)
    e = Entry(c["W"], c["u"], c["v"])
    _fwd_single(e, 0, c["eps"])
    R.check_iter0(c, e.results(0, "single"), "single")


CLAMPS = [((33, 257), -10, 24, False), ((70, 600), -10, 24, False), ((3, 27), 3, 10, True), ((33, 257), 3, 10, True), ((1, 5), -6, 24, True)]


@pytest.mark.parametrize("shape,k,s,u_clamped", CLAMPS)
def test_forward_eps_clamp_exact(shape, k, s, u_clamped):
    """|W^T u| < eps: v = W^T u / eps exactly; in the last three cases |W v| < eps too and u = W v / eps exactly."""
    c = R.clamp_case(*shape, 5, k, s)
    assert c["u_clamped"] == u_clamped
    e = Entry(c["W"], c["u"], c["v0"])
    _fwd_single(e, 1, c["eps"])
    R.check_clamp(c, e.results(1, "single"), "single")
    m = Entry(c["W"], c["u"], c["v0"], u_save=True, v_save=True)
    _fwd_multi([m], 1, c["eps"])
    R.check_clamp(c, m.results(1, "multi"), "multi")


def test_forward_zero_weight_is_nan_like_torch():
    rng = np.random.default_rng(0)
    for rows, cols in ((3, 27), (33, 257)):
        e = Entry(np.zeros((rows, cols), dtype=np.float32), rng.standard_normal(rows), rng.standard_normal(cols))
        _fwd_single(e, 1, 1e-12)
        R.check_zero(rows, cols, e.results(1, "single"), "single")
        m = Entry(np.zeros((rows, cols), dtype=np.float32), rng.standard_normal(rows), rng.standard_normal(cols))
        _fwd_multi([m], 1, 1e-12, save_arrays=False)
        R.check_zero(rows, cols, m.results(1, "multi"), "multi")


@pytest.mark.parametrize("rows,cols", R.POWER_SHAPES + R.NARROW_SHAPES)
def test_backward_exact(rows, cols):
    for a in (3, -2):
        b = BwdEntry(R.bwd_case(rows, cols, 9, a))
        _bwd_single(b)
        b.check(f"single sigma 2^{a}")


# ---------------------------------------------------------------------------------------------------------------------------------
# batched calls against the ORACLE (not the single path), exact tier
# ---------------------------------------------------------------------------------------------------------------------------------
# Mixed batches: the first entry is the smallest; the largest cols, the largest rows and the largest rows * cols are three different
# entries (the grids are sized by each maximum on its own, so no entry may own two of them).
BATCH16 = [(1, 5), (129, 1153), (3, 27), (260, 300), (2, 6), (257, 1025), (31, 255), (32, 256), (33, 257), (64, 27), (70, 600), (257, 40),
           (1, 512), (3, 27), (2, 6), (33, 257)]
BATCH4 = [(1, 5), (513, 1025), (600, 40), (129, 1153)]          # the second lap of the backward / dot caps inside a batch
BATCH1 = [(33, 257)]
BATCHES = {"n16": BATCH16, "n4": BATCH4, "n1": BATCH1}


def _assert_mixed(shapes):
    if len(shapes) < 3:
        return
    owners = {max(range(len(shapes)), key=lambda i: f(shapes[i])) for f in (lambda s: s[1], lambda s: s[0], lambda s: s[0] * s[1])}
    assert len(owners) == 3, "largest cols / rows / rows * cols must be three entries"
    assert shapes[0][0] * shapes[0][1] == min(r * c for r, c in shapes)


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("saves", ["arrays", "null_arrays", "null_entries"])
def test_forward_multi_power_iteration_exact(batch, saves):
    shapes = BATCHES[batch]
    _assert_mixed(shapes)
    cases = [R.power_case(r, c, 20 + i) for i, (r, c) in enumerate(shapes)]
    big = max(range(len(shapes)), key=lambda i: shapes[i][0] * shapes[i][1])
    es = []
    for i, c in enumerate(cases):
        save = saves == "arrays" or (saves == "null_entries" and i % 2 == 0)
        es.append(Entry(c["W"], c["u"], c["v0"], w_eff=(i % 3 != 1 or i == big), u_save=save, v_save=save and i % 4 != 0 or saves == "arrays"))
    _fwd_multi(es, 1, 1e-12, save_arrays=saves != "null_arrays")
    for i, (c, e) in enumerate(zip(cases, es)):
        R.check_power(c, e.results(1, f"multi[{i}]"), f"multi[{i}]")


@pytest.mark.parametrize("batch", list(BATCHES))
def test_forward_multi_without_power_iteration_exact(batch):
    shapes = list(BATCHES[batch])
    if len(shapes) == 16:
        shapes[13], shapes[14] = (4, 1), (9, 3)
        shapes[0], shapes[13] = shapes[13], shapes[0]                # the smallest first
    _assert_mixed(shapes)
    cases = [R.iter0_case(r, c, 40 + i) for i, (r, c) in enumerate(shapes)]
    big = max(range(len(shapes)), key=lambda i: shapes[i][0] * shapes[i][1])
    es = [Entry(c["W"], c["u"], c["v"], w_eff=(i % 3 != 2 or i == big), u_save=i % 2 == 0, v_save=i % 3 != 0) for i, c in enumerate(cases)]
    _fwd_multi(es, 0, 1e-12)
    for i, (c, e) in enumerate(zip(cases, es)):
        R.check_iter0(c, e.results(0, f"multi[{i}]"), f"multi[{i}]")


@pytest.mark.parametrize("batch", list(BATCHES))
def test_backward_multi_exact(batch):
    shapes = BATCHES[batch]
    _assert_mixed(shapes)
    bs = [BwdEntry(R.bwd_case(r, c, 60 + i, (3, -2, 0)[i % 3])) for i, (r, c) in enumerate(shapes)]
    _bwd_multi(bs)
    for i, b in enumerate(bs):
        b.check(f"multi[{i}]")


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections: RuntimeError, nothing written
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing():
    c = R.iter0_case(3, 27, 3)

    def fresh(n):
        return [Entry(c["W"], c["u"], c["v"], u_save=True, v_save=True) for _ in range(n)]

    def untouched(es, what):
        for e in es:
            for key in ("sigma", "w_eff", "u_save", "v_save", "scratch"):
                getattr(e, key).untouched(f"{what}: {key}")
            assert np.array_equal(e.u.numpy(what), c["u"]) and np.array_equal(e.v.numpy(what), c["v"]), f"{what}: u / v"

    lib = _lib()
    for power_iter in (0, 1):
        # n = 0 and n = 17 (the arrays hold 17 valid entries: only the count is wrong)
        es = fresh(17)
        for n in (0, 17):
            opt = lambda key: _P([getattr(e, key).ptr for e in es])  # noqa: E731
            with pytest.raises(RuntimeError):
                lib.call("wu_spectral_norm_fwd_multi", n, _P([e.W.ptr for e in es]), _I([3] * 17), _I([27] * 17), opt("u"), opt("v"), power_iter,
                         1e-12, opt("sigma"), opt("w_eff"), opt("scratch"), opt("u_save"), opt("v_save"), _stream())
        torch.cuda.synchronize()
        untouched(es, f"n = 0 / 17, power_iter {power_iter}")
        # rows = 0 and cols = 256 * 1024 + 1, single call and as the second entry of a batch
        wide = 256 * 1024 + 1
        big = Entry(np.ones((1, wide), dtype=np.float32), np.ones(1), np.ones(wide), w_eff=True, u_save=True, v_save=True)
        for rows, cols, e in ((0, 27, fresh(1)[0]), (1, wide, big)):
            ok = fresh(1)[0]
            with pytest.raises(RuntimeError):
                lib.call("wu_spectral_norm_fwd", e.W.ptr, rows, cols, e.u.ptr, e.v.ptr, power_iter, 1e-12, e.sigma.ptr, e.w_eff.ptr, e.scratch.ptr,
                         _stream())
            with pytest.raises(RuntimeError):
                pair = [ok, e]
                opt = lambda key: _P([getattr(x, key).ptr for x in pair])  # noqa: E731
                lib.call("wu_spectral_norm_fwd_multi", 2, _P([x.W.ptr for x in pair]), _I([3, rows]), _I([27, cols]), opt("u"), opt("v"), power_iter,
                         1e-12, opt("sigma"), opt("w_eff"), opt("scratch"), opt("u_save"), opt("v_save"), _stream())
            torch.cuda.synchronize()
            untouched([ok], f"rows {rows} cols {cols}: the valid first entry")
            for key in ("sigma", "w_eff", "u_save", "v_save", "scratch"):
                getattr(e, key).untouched(f"rows {rows} cols {cols}: {key}")
    # backward: n = 0, n = 17, rows = 0
    bs = [BwdEntry(R.bwd_case(3, 27, 9, 0)) for _ in range(17)]
    col = lambda k: _P([b.inputs[k].ptr for b in bs])  # noqa: E731
    for n in (0, 17):
        with pytest.raises(RuntimeError):
            lib.call("wu_spectral_norm_bwd_multi", n, col("G"), col("W"), col("u"), col("v"), col("sigma"), _P([b.dw.ptr for b in bs]),
                     _I([3] * 17), _I([27] * 17), _P([b.scratch.ptr for b in bs]), _stream())
    b = bs[0]
    i = b.inputs
    with pytest.raises(RuntimeError):
        lib.call("wu_spectral_norm_bwd", i["G"].ptr, i["W"].ptr, i["u"].ptr, i["v"].ptr, i["sigma"].ptr, b.dw.ptr, 0, 27, b.scratch.ptr, _stream())
    torch.cuda.synchronize()
    for b in bs:
        b.dw.untouched("backward rejection: dw")
        b.scratch.untouched("backward rejection: scratch")


# ---------------------------------------------------------------------------------------------------------------------------------
# tolerance tier: wu.functional against stock spectral_norm in float64
# ---------------------------------------------------------------------------------------------------------------------------------
# weight shapes as the modules hold them (rows = shape[0]): 4x1, 9x3, 3x27, 1x512, 33x257, 70x600, 64x27
TOL_SHAPES = [(4, 1), (9, 3), (3, 3, 3, 3), (1, 512), (33, 257), (70, 600), (64, 3, 3, 3)]


def _gauss(shape, seed):
    rng = np.random.default_rng(seed)
    rows, cols = shape[0], int(np.prod(shape[1:]))
    W = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    u, v = rng.standard_normal(rows), rng.standard_normal(cols)
    return W, (u / np.linalg.norm(u)).astype(np.float32), (v / np.linalg.norm(v)).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("multi", [False, True])
def test_training_and_eval_steps_inside_the_running_error_bound(multi):
    """Three training forwards (the buffers advance in place) and one eval forward, a backward each time.  Before every step the
    float64 stock module takes the buffers the kernels are about to read, so each step is one application of the operation to identical
    inputs and the bounds of _sn_ref hold per step.  In the batched run the weights 1 and 4 are frozen (requires_grad = False): the
    backward runs over the subset and they get no gradient."""
    from wu import functional as WF
    dev = _dev()
    data = [_gauss(s, 30 + i) for i, s in enumerate(TOL_SHAPES)]
    frozen = {1, 4} if multi else set()
    ws = [torch.from_numpy(W).to(dev).requires_grad_(i not in frozen) for i, (W, _, _, _) in enumerate(data)]
    us = [torch.from_numpy(u).to(dev) for _, u, _, _ in data]
    vs = [torch.from_numpy(v).to(dev) for _, _, v, _ in data]
    gs = [torch.from_numpy(G).to(dev) for _, _, _, G in data]
    stock = [R.StockSN(W.reshape(W.shape[0], -1), 1e-12) for W, _, _, _ in data]
    worst = 0.0
    for step, train in enumerate((True, True, True, False)):
        before = [(u.cpu().numpy(), v.cpu().numpy()) for u, v in zip(us, vs)]
        for w in ws:
            w.grad = None
        if multi:
            outs = WF.spectral_normalize_multi(ws, us, vs, train, 1e-12)
        else:
            outs = [WF.spectral_normalize(w, u, v, train, 1e-12) for w, u, v in zip(ws, us, vs)]
        torch.autograd.backward(list(outs), gs)
        torch.cuda.synchronize()
        for i, (W, _, _, G) in enumerate(data):
            W2, G2 = W.reshape(W.shape[0], -1), G.reshape(W.shape[0], -1)
            u0, v0 = before[i]
            ref = stock[i].step(u0, v0, train, G2)
            fb = R.forward_bounds(W2, u0, v0, train)
            got = dict(w_eff=outs[i].detach().cpu().numpy(), u=us[i].cpu().numpy(), v=vs[i].cpu().numpy())
            assert np.array_equal(ws[i].detach().cpu().numpy(), W), "weight modified"
            if i in frozen:
                assert ws[i].grad is None
                bb = None
            else:
                got["dw"] = ws[i].grad.cpu().numpy()
                bb = R.backward_bounds(G2, W2, fb)
            worst = max(worst, R.check_tolerance(f"{'multi' if multi else 'single'} {TOL_SHAPES[i]} step {step}", ref, fb, got, bb))
    print(f"worst observed / bound over all steps: {worst:.3f}")
