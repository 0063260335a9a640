"""The kernels only the TRAINABLE ResNet-101 runs -- bn_stats_*, bn_apply_kernel, bn_bwd_*, pw_wgrad_kernel, stem_wgrad_kernel, slab_fold_kernel
(csrc/resnet_train.hip) and maxpool3s2_fwd/bwd_kernel (csrc/resnet.hip) -- through the C ABI against the exact CPU oracles of
tests/_train_ref.py.

Every comparison is a torch.equal, except two that cannot be: running_var (n / (n - 1) and one fp32 multiply-add: 2 fp32 ulps of the
float64 value) and dx where M is not a power of two (1 / M is rounded: the bound derived at _train_ref.dx_bound, on every element).
tests/test_train_ref_cpu.py proves the premises per case; the cheap ones are asserted again next to the launch.  Every activation-sized
operand and result is the middle channel slice of a NaN-filled buffer with GUARD channels on either side, every per-channel result and
weight gradient sits between NaN guard words, every workspace is NaN-filled, exactly as large as the library asks for, and followed by
guard words; all of them are looked at after the launch.  Each kernel gets the ORACLE's inputs (statistics, stored output y, arg-max), so
one wrong kernel fails its own comparison only."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _train_ref as R
from test_gpu_conv_walk import GUARD, _check_slice, _dev, _exact, _sliced
from test_gpu_pointwise_exact import _put

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _code(dtype):
    from wu import _lib
    return _lib.BF16 if dtype == "bf16" else _lib.F32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows(t):
    """(M, C) rows on the CPU -> (1, C, 1, M)."""
    return t.t()[None, :, None, :].contiguous()


def _put_nan(t, dtype, lead=GUARD, trail=GUARD):
    """_put for a tensor that holds NaN on purpose (the lossless check ignores those sites)."""
    n, c, h, w = t.shape
    buf = torch.full((n, h, w, lead + c + trail), NAN, dtype=dtype, device=_dev()).permute(0, 3, 1, 2)
    s = buf[:, lead:lead + c]
    s.copy_(t.to(_dev()))
    assert torch.equal(s.float().cpu().nan_to_num(nan=12345.0), t.nan_to_num(nan=12345.0))
    return s


def _untouched(s, t, what, lead=GUARD):
    """An input slice still holds `t` and the channels around it are still NaN."""
    base, c = s._base, t.shape[1]
    assert torch.equal(s.float().cpu().nan_to_num(nan=12345.0), t.nan_to_num(nan=12345.0)), f"{what}: an input changed"
    assert bool(torch.isnan(base[..., :lead]).all()) and bool(torch.isnan(base[..., lead + c:]).all()), f"{what}: wrote beside an input"


def _guarded(n, dtype=torch.float32, fill=NAN):
    """n values between GUARD guard values, all `fill`."""
    full = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=_dev())
    return full, full[GUARD:GUARD + n]


def _guards_ok(full, what, fill=NAN):
    for g in (full[:GUARD], full[-GUARD:]):
        assert bool(torch.isnan(g).all() if fill != fill else (g == fill).all()), f"{what}: wrote outside its buffer"


def _workspace(nbytes):
    """A NaN-filled workspace of exactly the size the library asks for, followed by guard words."""
    assert nbytes > 0 and nbytes % 4 == 0
    full = torch.full((nbytes // 4 + GUARD,), NAN, dtype=torch.float32, device=_dev())
    assert full.data_ptr() % 16 == 0
    return full, nbytes


def _workspace_ok(full, nbytes, what):
    assert bool(torch.isnan(full[nbytes // 4:]).all()), f"{what}: wrote beyond the workspace size it asked for"
    assert not bool(torch.isnan(full[:nbytes // 4]).any()), f"{what}: read the result from workspace words no kernel wrote"


def _vec(t):
    return t.float().contiguous().to(_dev())


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _bn_reference(name):
    case = R.BN_BY_NAME[name]
    ops = R.bn_operands(case)
    sts = []
    for b in (ops["b1"], ops["b2"]):
        if b is None:
            sts.append(None)
            continue
        mean, var, rstd = R.bn_stats_reference(case, b)
        for bound in R.stats_bounds(b["x"]):
            _exact(bound)
        sts.append(dict(mean=mean, var=var, rstd=rstd, t=R.stats_tensor(mean, rstd)))
    s1 = (sts[0]["mean"], sts[0]["rstd"])
    s2 = (sts[1]["mean"], sts[1]["rstd"]) if sts[1] else None
    lin, out = R.bn_apply_reference(case, ops, s1, s2)
    return ops, sts, s1, s2, lin, out


BN_PARAMS = [pytest.param(c, d, id=f"{c.name}-{d}") for c in R.BN_CASES for d in c.dtypes]
# the exact LeakyReLU apply stores fp32 (_train_ref: 0.2f v is the kernel's one fp32 multiply, kept whole only by an fp32 output)
BN_APPLY_PARAMS = [pytest.param(c, d, id=f"{c.name}-{d}") for c in R.BN_CASES for d in c.dtypes if not (c.act == R.LEAKY and d == "bf16")]


@pytest.mark.parametrize("case,dtype", BN_PARAMS)
def test_bn_stats_is_exact(case, dtype):
    """bn_stats_partial_kernel + bn_stats_final_kernel: mean, rstd, running_mean and num_batches_tracked bit for bit; running_var within
    2 fp32 ulps of the float64 value.  One split, even splits, an uneven last split, an EMPTY last split, the 256-split clamp; fewer rows
    than a workgroup keeps in flight; the second and third 64-channel group."""
    from wu import _lib
    ops, sts, _, _, _, _ = _bn_reference(case.name)
    assert R.bn_plan(case.m, case.c, dtype)[::2] == case.plan[dtype]
    dt, b, ref = R.TORCH_DTYPE[dtype], ops["b1"], sts[0]
    x = _put(_rows(b["x"]), dt, lead=GUARD, trail=GUARD)
    need = _lib.load().wu_bn_stats_workspace(case.m, case.c, _code(dtype))
    assert need == R.bn_workspace_floats(case.m, case.c, dtype, 2) * 4
    ws, nbytes = _workspace(need)
    sfull, st = _guarded(2 * case.c)
    rmfull, rm = _guarded(case.c)
    rvfull, rv = _guarded(case.c)
    rm.copy_(ops["running_mean0"])
    rv.copy_(ops["running_var0"])
    tracked = torch.tensor([7, ops["tracked0"], 7], dtype=torch.int64, device=_dev())
    what = f"bn_stats {case.name} {dtype}"
    _lib.call("wu_bn_stats", x.data_ptr(), x.stride(3), case.m, case.c, case.eps, case.momentum, st.data_ptr(), rm.data_ptr(), rv.data_ptr(),
              tracked[1:].data_ptr(), ws.data_ptr(), nbytes, _code(dtype), _stream())
    want_rm, want_rv = R.running_reference(case, ops, ref["mean"], ref["var"])
    got = st.cpu()
    assert torch.equal(got[:case.c], ref["t"][0]), f"{what}: mean differs on channels {(got[:case.c] != ref['t'][0]).nonzero().flatten().tolist()[:8]}"
    assert torch.equal(got[case.c:], ref["t"][1]), f"{what}: rstd differs on channels {(got[case.c:] != ref['t'][1]).nonzero().flatten().tolist()[:8]}"
    assert torch.equal(rm.cpu(), want_rm), f"{what}: running_mean"
    assert tracked.tolist() == [7, ops["tracked0"] + 1, 7], f"{what}: num_batches_tracked"
    err = (rv.cpu().double() - want_rv).abs() / R.ulp32(want_rv)
    print(f"{what}: running_var off by at most {float(err.max()):.3f} fp32 ulps (bound {R.RUNNING_VAR_ULPS})")
    assert bool((err <= R.RUNNING_VAR_ULPS).all()), f"{what}: running_var {float(err.max())} ulps off"
    for full in (sfull, rmfull, rvfull):
        _guards_ok(full, what)
    _workspace_ok(ws, nbytes, what)
    _untouched(x, _rows(b["x"]), what)


@pytest.mark.parametrize("case,dtype", BN_APPLY_PARAMS)
def test_bn_apply_is_exact(case, dtype):
    """bn_apply_kernel, single / dual / residual, no activation / ReLU / LeakyReLU (the latter stores fp32: _train_ref), against the exact
    dyadic value rounded ONCE; the last case walks the grid-stride loop twice."""
    from wu import _lib
    ops, sts, _, _, lin, out = _bn_reference(case.name)
    dt = R.TORCH_DTYPE[dtype]
    if case.act != R.NONE:
        assert int((lin == 0).sum()) > 0
    if dtype == "bf16" and case.form == "res":
        assert R.unrepresentable(out) >= 0.01
    if "gridstride" in case.name:
        assert case.m * (case.c // R.VEC[dtype]) > 256 * 32 * 256
    b1, b2 = ops["b1"], ops["b2"]
    ins = {"x": _rows(b1["x"])}
    if b2 is not None:
        ins["x2"] = _rows(b2["x"])
    if ops["res"] is not None:
        ins["res"] = _rows(ops["res"])
    dev = {k: _put(v, dt, lead=GUARD, trail=GUARD) for k, v in ins.items()}
    st1, g1, be1 = sts[0]["t"].to(_dev()), _vec(b1["gamma"]), _vec(b1["beta"])
    st2, g2, be2 = (sts[1]["t"].to(_dev()), _vec(b2["gamma"]), _vec(b2["beta"])) if b2 is not None else (None, None, None)
    buf, y = _sliced(1, case.c, 1, case.m, dtype=dt)
    ptr = lambda t: t.data_ptr() if t is not None else None         # noqa: E731
    ld = lambda k: dev[k].stride(3) if k in dev else 0               # noqa: E731
    what = f"bn_apply {case.name} {dtype} [{case.form}, act {case.act}]"
    _lib.call("wu_bn_apply", dev["x"].data_ptr(), ld("x"), st1.data_ptr(), g1.data_ptr(), be1.data_ptr(), ptr(dev.get("x2")), ld("x2"), ptr(st2),
              ptr(g2), ptr(be2), ptr(dev.get("res")), ld("res"), y.data_ptr(), y.stride(3), case.m, case.c, case.act, _code(dtype), _stream())
    _check_slice(buf, case.c, _rows(out).to(dt).to(_dev()), what)
    for k, v in ins.items():
        _untouched(dev[k], v, f"{what}: {k}")


@pytest.mark.parametrize("case,dtype", BN_PARAMS)
def test_bn_bwd_is_exact(case, dtype):
    """bn_bwd_partial_kernel + bn_bwd_final_kernel + bn_bwd_dx_kernel from the oracle's stored output y (exact zeros: the gate at
    y == 0), without y, with gres, dual (dbeta2 == dbeta): dbeta, dgamma and gres bit for bit for any M; dx and dx2 bit for bit where M is a
    power of two, inside the derived bound on every element elsewhere.  Under the LeakyReLU gate 0.2f g is not dyadic: gres alone."""
    from wu import _lib
    ops, sts, s1, s2, lin, out = _bn_reference(case.name)
    dt = R.TORCH_DTYPE[dtype]
    y_cpu = None if case.act == R.NONE else out.to(dt)
    ref = R.bn_bwd_reference(case, ops, y_cpu, s1, s2)
    if y_cpu is not None:
        assert int((y_cpu == 0).sum()) > 0
    if "gridstride" in case.name:
        assert case.m * (case.c // R.VEC[dtype]) > 256 * 32 * 256
    b1, b2 = ops["b1"], ops["b2"]
    ins = {"g": _rows(ops["g"]), "x": _rows(b1["x"])}
    if y_cpu is not None:
        ins["y"] = _rows(y_cpu.float())
    if b2 is not None:
        ins["x2"] = _rows(b2["x"])
    dev = {k: _put(v, dt, lead=GUARD, trail=GUARD) for k, v in ins.items()}
    st1, g1 = sts[0]["t"].to(_dev()), _vec(b1["gamma"])
    st2, g2 = (sts[1]["t"].to(_dev()), _vec(b2["gamma"])) if b2 is not None else (None, None)
    outs = {k: _guarded(case.c) for k in (("dgamma", "dbeta", "dgamma2", "dbeta2") if b2 is not None else ("dgamma", "dbeta"))}
    dxb, dx = _sliced(1, case.c, 1, case.m, dtype=dt)
    dx2b, dx2 = _sliced(1, case.c, 1, case.m, dtype=dt) if b2 is not None else (None, None)
    grb, gres = _sliced(1, case.c, 1, case.m, dtype=dt) if case.gres else (None, None)
    need = _lib.load().wu_bn_bwd_workspace(case.m, case.c, _code(dtype))
    assert need == R.bn_workspace_floats(case.m, case.c, dtype, 3) * 4
    ws, nbytes = _workspace(need)
    ptr = lambda t: t.data_ptr() if t is not None else None         # noqa: E731
    ld = lambda t: t.stride(3) if t is not None else 0               # noqa: E731
    o = lambda k: outs[k][1].data_ptr() if k in outs else None      # noqa: E731
    what = f"bn_bwd {case.name} {dtype} [{case.form}, gate {case.act}]"
    _lib.call("wu_bn_bwd", dev["g"].data_ptr(), ld(dev["g"]), ptr(dev.get("y")), ld(dev.get("y")), case.act, dev["x"].data_ptr(), ld(dev["x"]),
              st1.data_ptr(), g1.data_ptr(), o("dgamma"), o("dbeta"), dx.data_ptr(), ld(dx), ptr(dev.get("x2")), ld(dev.get("x2")), ptr(st2), ptr(g2),
              o("dgamma2"), o("dbeta2"), ptr(dx2), ld(dx2), ptr(gres), ld(gres), case.m, case.c, ws.data_ptr(), nbytes, _code(dtype), _stream())
    failures = []

    def check(fn):
        try:
            fn()
        except AssertionError as e:
            failures.append(str(e))

    if case.gres:
        check(lambda: _check_slice(grb, case.c, _rows(ref["gg"]).to(dt).to(_dev()), f"{what}: gres"))
    if case.act != R.LEAKY:
        def per_channel(name, want64):
            got = outs[name][1].cpu()
            assert torch.equal(got, want64.float()), f"{what}: {name} differs on channels {(got != want64.float()).nonzero().flatten().tolist()[:8]}"
        check(lambda: per_channel("dbeta", ref["dbeta"]))
        check(lambda: per_channel("dgamma", ref["dgamma"]))
        if b2 is not None:
            check(lambda: per_channel("dbeta2", ref["dbeta"]))
            check(lambda: per_channel("dgamma2", ref["dgamma2"]))
            assert torch.equal(outs["dbeta2"][1], outs["dbeta"][1]), f"{what}: dbeta2 != dbeta"
        for key, buf in (("", dxb), ("2", dx2b)):
            if buf is None:
                continue
            want = ref["dx" + key]
            if R.is_pow2(case.m):
                assert torch.equal(want.float().double(), want)
                check(lambda: _check_slice(buf, case.c, _rows(want.float()).to(dt).to(_dev()), f"{what}: dx{key}"))
            else:
                got = buf[:, GUARD:GUARD + case.c].float().cpu()[0, :, 0, :].t().double()
                bound = R.dx_bound(ref, key, dtype, case.m)
                err = (got - want).abs()
                over = (err > bound) | torch.isnan(got)
                print(f"{what}: dx{key} largest error / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f} over {err.numel()} elements")
                if bool(over.any()):
                    failures.append(f"{what}: dx{key}: {int(over.sum())} of {over.numel()} elements outside the derived bound; first (row, channel) = "
                                    f"{over.nonzero()[0].tolist()}, error {float(err[over].max()):.3e}")
                assert bool(torch.isnan(buf[:, :GUARD]).all()) and bool(torch.isnan(buf[:, GUARD + case.c:]).all()), f"{what}: dx{key} wrote outside its slice"
    else:
        for buf in (dxb, dx2b):
            if buf is not None:
                assert bool(torch.isnan(buf[:, :GUARD]).all()) and bool(torch.isnan(buf[:, GUARD + case.c:]).all()), f"{what}: dx wrote outside its slice"
    for full, _ in outs.values():
        _guards_ok(full, what)
    _workspace_ok(ws, nbytes, what)
    for k, v in ins.items():
        _untouched(dev[k], v, f"{what}: {k}")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.PW_WGRAD_CASES, ids=lambda c: c.name)
def test_conv1x1_wgrad_is_exact(c):
    """pw_wgrad_kernel + slab_fold_kernel in bf16 and fp32: fewer rows than a K stage, one stage, one more row, two splits with a ragged
    second, the 64-split cap; square and rectangular tile grids (a mismatch is reported by tile); the stride-2 gather with NaN at every
    pixel it must skip; written into NaN and accumulated onto integers."""
    from wu import _lib
    m = c.n * c.hc * c.wc
    req, splits, rps = R.pw_wgrad_plan(m, c.cin, c.cout)
    assert (req, splits, rps, m - (splits - 1) * rps) == c.plan
    _exact(R.pw_wgrad_bound(c))
    ops = R.pw_wgrad_operands(c)
    want = R.pw_wgrad_reference(c, ops)
    need = _lib.load().wu_conv1x1_wgrad_workspace(m, c.cin, c.cout)
    assert need == splits * c.cout * c.cin * 4
    failures = []
    for dtype in ("bf16", "fp32"):
        dt = R.TORCH_DTYPE[dtype]
        x, dy = _put_nan(ops["x"], dt), _put(ops["dy"], dt, lead=GUARD, trail=2 * GUARD)
        full, dw = _guarded(c.cout * c.cin)
        if c.accumulate:
            dw.copy_(ops["dw0"].flatten())
        ws, nbytes = _workspace(need)
        what = f"conv1x1_wgrad {c.name} {dtype}"
        _lib.call("wu_conv1x1_wgrad", x.data_ptr(), x.stride(3), dy.data_ptr(), dy.stride(3), dw.data_ptr(), ws.data_ptr(), nbytes, c.n, c.hc, c.wc,
                  c.in_stride, c.hin, c.win, c.cin, c.cout, 1 if c.accumulate else 0, _code(dtype), _stream())
        bad = R.tiles_that_differ(dw.cpu().view(c.cout, c.cin), want)
        if bad:
            failures.append(f"{what}: (cout tile, cin tile, elements) that differ from the CPU integer oracle: {bad[:12]}")
        _guards_ok(full, what)
        _workspace_ok(ws, nbytes, what)
        _untouched(x, ops["x"], f"{what}: x")
        _untouched(dy, ops["dy"], f"{what}: dy")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("c", R.STEM_WGRAD_CASES, ids=lambda c: c.name)
def test_stem7x7_wgrad_is_exact(c):
    """stem_wgrad_kernel + slab_fold_kernel with bf16 and fp32 gradients: a one-pixel image, fewer pixels than a 32-pixel stage, ragged
    last stages and splits, the 512-split cap; the image between NaN images, the gradient a slice of a wider buffer, the workspace and dw
    in NaN (the padding taps and the tap >= 147 lanes of the last group have nowhere to hide)."""
    from wu import _lib
    assert R.stem_wgrad_plan(c.n, c.h, c.w) == c.plan
    _exact(R.stem_wgrad_bound(c))
    ops = R.stem_wgrad_operands(c)
    want = R.stem_wgrad_reference(c, ops)
    need = _lib.load().wu_stem7x7_wgrad_workspace(c.n, c.h, c.w)
    assert need == c.plan[0] * 64 * R.ST_TAPS * 4
    images = torch.full((c.n + 2, 3, c.h, c.w), NAN, device=_dev())
    x = images[1:c.n + 1]
    x.copy_(ops["x"])
    failures = []
    for dtype in ("bf16", "fp32"):
        dt = R.TORCH_DTYPE[dtype]
        dy = _put(ops["dy"], dt, lead=GUARD, trail=GUARD)
        full, dw = _guarded(64 * R.ST_TAPS)
        if c.accumulate:
            dw.copy_(ops["dw0"].flatten())
        ws, nbytes = _workspace(need)
        what = f"stem7x7_wgrad {c.name} {dtype}"
        _lib.call("wu_stem7x7_wgrad", x.data_ptr(), dy.data_ptr(), dy.stride(3), dw.data_ptr(), ws.data_ptr(), nbytes, c.n, c.h, c.w,
                  1 if c.accumulate else 0, _code(dtype), _stream())
        got = dw.cpu().view(64, 3, 7, 7)
        if not torch.equal(got, want):
            bad = ((got != want) | torch.isnan(got)).nonzero()
            failures.append(f"{what}: {len(bad)} of {got.numel()} elements differ from the CPU integer oracle; first (co, ci, kh, kw) = {bad[0].tolist()}, "
                            f"last = {bad[-1].tolist()}")
        _guards_ok(full, what)
        _workspace_ok(ws, nbytes, what)
        _untouched(dy, ops["dy"], f"{what}: dy")
    assert torch.equal(x.cpu(), ops["x"]) and bool(torch.isnan(images[0]).all()) and bool(torch.isnan(images[-1]).all())
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# maxpool3s2
# ---------------------------------------------------------------------------------------------------------------------------------
IDX_FILL = 0xAB


@functools.lru_cache(maxsize=1)
def _pool_reference(c):
    ops = R.pool_operands(c)
    y, am = R.pool_forward_restatement(ops["x"])
    ty, tdx = (F.max_pool2d(ops["x"], 3, 2, 1), None) if c.nans else R.pool_autograd(ops["x"], ops["dy"])
    assert torch.equal(y.nan_to_num(nan=12345.0), ty.nan_to_num(nan=12345.0))
    return ops, ty, am, tdx


def _run_pool_forward(c):
    from wu import _lib
    ops, ty, am, _ = _pool_reference(c)
    dt = R.TORCH_DTYPE[c.dtype]
    ho, wo = R.stem_out(c.h, c.w)
    x = _put_nan(ops["x"], dt)
    buf, y = _sliced(c.n, c.c, ho, wo, dtype=dt)
    ifull, idx = _guarded(c.n * ho * wo * c.c, dtype=torch.uint8, fill=IDX_FILL)
    what = f"maxpool3s2_fwd {c.name}"
    _lib.call("wu_maxpool3s2_fwd", x.data_ptr(), x.stride(3), y.data_ptr(), y.stride(3), idx.data_ptr(), c.n, c.h, c.w, c.c, _code(c.dtype), _stream())
    want = ty.to(dt).to(_dev())
    if c.nans:
        got = buf[:, GUARD:GUARD + c.c]
        assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN where torch has none, or the reverse"
        assert torch.equal(got.nan_to_num(nan=12345.0), want.nan_to_num(nan=12345.0)), f"{what}: differs from F.max_pool2d"
        assert bool(torch.isnan(buf[:, :GUARD]).all()) and bool(torch.isnan(buf[:, GUARD + c.c:]).all()), f"{what}: wrote outside its channel slice"
    else:
        _check_slice(buf, c.c, want, what)
    got_idx = idx.cpu().view(c.n, ho, wo, c.c)
    if not torch.equal(got_idx, am):
        bad = (got_idx != am).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {am.numel()} arg-max bytes differ from 'first maximum in scan order'; first (n, oh, ow, c) = "
                             f"{bad[0].tolist()}: stored {int(got_idx[tuple(bad[0])])}, want {int(am[tuple(bad[0])])}")
    _guards_ok(ifull, what, fill=IDX_FILL)
    _untouched(x, ops["x"], what)


def _run_pool_backward(c):
    from wu import _lib
    ops, _, am, tdx = _pool_reference(c)
    dt = R.TORCH_DTYPE[c.dtype]
    ho, wo = R.stem_out(c.h, c.w)
    dy = _put(ops["dy"], dt, lead=GUARD, trail=GUARD)
    x = _put(ops["x"], dt, lead=GUARD, trail=2 * GUARD)
    ifull, idx = _guarded(c.n * ho * wo * c.c, dtype=torch.uint8, fill=IDX_FILL)
    idx.copy_(am.flatten())
    failures = []
    for label, gate, xg, want in (("ungated, x = NULL", R.NONE, None, tdx),
                                  ("ReLU-gated", R.RELU, x, torch.where(ops["x"] > 0, tdx, torch.zeros_like(tdx)))):
        buf, dx = _sliced(c.n, c.c, c.h, c.w, dtype=dt)
        what = f"maxpool3s2_bwd {c.name} [{label}]"
        _lib.call("wu_maxpool3s2_bwd", dy.data_ptr(), dy.stride(3), idx.data_ptr(), xg.data_ptr() if xg is not None else None,
                  xg.stride(3) if xg is not None else 0, dx.data_ptr(), dx.stride(3), c.n, c.h, c.w, c.c, gate, _code(c.dtype), _stream())
        assert torch.equal(want.to(dt).float(), want)                # sums of at most four integers of [-4, 4]
        try:
            _check_slice(buf, c.c, want.to(dt).to(_dev()), what)
        except AssertionError as e:
            failures.append(str(e))
    assert torch.equal(idx.cpu(), am.flatten())
    _guards_ok(ifull, "maxpool3s2_bwd", fill=IDX_FILL)
    _untouched(dy, ops["dy"], "maxpool3s2_bwd: dy")
    _untouched(x, ops["x"], "maxpool3s2_bwd: x")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("c", R.POOL_CASES, ids=lambda c: c.name)
def test_maxpool3s2_forward_and_argmax_are_exact(c):
    """The output equals F.max_pool2d bit for bit (NaN exactly where torch has NaN) and the stored arg-max bytes equal the restated rule,
    first maximum in scan order over the in-bounds taps: on integers of [-2, 2], where most windows tie."""
    _run_pool_forward(c)


@pytest.mark.parametrize("c", [c for c in R.POOL_CASES if not c.nans], ids=lambda c: c.name)
def test_maxpool3s2_backward_is_exact(c):
    """The gather backward, ungated as the training path calls it and ReLU-gated with zeros in x, equals autograd of F.max_pool2d (which
    routes ties to the same tap as the restated arg-max: tests/test_train_ref_cpu.py)."""
    _run_pool_backward(c)


def test_maxpool3s2_grid_stride_loops():
    """Shapes with more 16-byte vectors than grid_cap's 256 * 16 workgroups of 256 threads: the forward over its output, the backward over
    its input."""
    f, b = R.POOL_FWD_BIG, R.POOL_BWD_BIG
    ho, wo = R.stem_out(f.h, f.w)
    assert f.n * ho * wo * f.c // R.VEC[f.dtype] > 256 * 16 * 256
    assert b.n * b.h * b.w * b.c // R.VEC[b.dtype] > 256 * 16 * 256
    _run_pool_forward(f)
    _run_pool_backward(b)
