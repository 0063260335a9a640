"""The generic 3 x 3 weight gradient (csrc/conv3x3_wgrad.hip) against the EXACT CPU integer oracle of tests/_wgrad_ref.py, beyond the one
instance tests/test_gpu_conv_walk.py pins (bf16, stride 1, images wider than 16 pixels):

  conv3x3_wgrad_kernel<bf16_t,2,128>   the register prefetch through per-image buffer descriptors, padding by out-of-range offsets and
                                       border flags, the fa_off / fb_off / tap_off tables, the hand-pipelined 72 MFMAs
  conv3x3_wgrad_kernel<float,1,128>    mfma_f32_32x32x2f32 fragments from 256-byte LDS rows
  conv3x3_wgrad_kernel<float,2,64>     the stride-2 prefetch with NX = 21, ND = 4 and the fp32 fragment loop on the 4x-strided halo
  conv3x3_wgrad_kernel<bf16_t,1,256>   at tile widths 16, 8 and 4 (Wo <= 16)
  wgrad_reduce_kernel                  at wpr 1 / 2 / 4 / 8, with empty split groups, odd and even splits per group, two c4b trips
  act_gate_kernel (wu_act_gate), the in-kernel gate (y != NULL) and the y-gated upsample_zero_gate_kernel of wu_conv3x3_s2_dgrad

Operands are small integers, so the fp32 sums are exact in any order and every tile, split and reducer tree must give the SAME bits:
torch's CPU fp32 conv2d_weight.  Every comparison is a torch.equal, except the derived-bound one of the fp32 LeakyReLU gate (0.2f dy is no
short dyadic number).  tests/test_wgrad_ref_cpu.py proves for every case here that the bound holds, that fp32 equals float64, that the plan
features a case is there for hold, and that the operands can see a wrong border rule; the features are asserted again next to the launch.

x, dy and y are channel slices of wider NaN-filled NHWC buffers with pairwise different pixel strides, and NaN-filled guard images lie in
front of the first and behind the last image: whatever the stride-2 descriptors (base one row and one pixel BEFORE the image, rows below it
meant to fall off num_records) let through from outside the tensor poisons the result.  All of it is memory the test owns.

The three shapes of test_conv3x3_wgrad_generic_is_exact give one tile per split (asserted in test_wgrad_ref_cpu.py); the multi-tile loop of
<bf16_t,1,256> is walked by the 224 x 224 layer test (512 -> 512 at 28 x 28: 8 tiles per split), that of the other three instances by the
45 x 79 cases here."""
import functools

import pytest
import torch

import _pointwise_ref as PR
import _wgrad_ref as R
from test_gpu_conv_walk import GUARD, _check_slice, _cu_count, _dev, _exact, _sliced
from test_gpu_pointwise_exact import TORCH_DTYPE, _options, _put, _rounded

pytestmark = pytest.mark.gpu

OPT_GRID = 10
ACT_NAME = {R.NONE: "ungated", R.RELU: "relu", R.LEAKY: "leaky"}


def _code(dtype):
    from wu import _lib
    return _lib.BF16 if dtype == "bf16" else _lib.F32


def _put_guarded(t, dtype, lead=0, trail=0):
    """`_put`, with NaN-filled guard images in front of the first and behind the last image: at least one image row and two pixels, what
    the stride-2 descriptor base lies before the image."""
    n, _, h, w = t.shape
    g = -(-(w + 2) // (h * w))
    zeros = torch.zeros((g,) + tuple(t.shape[1:]))
    s = _put(torch.cat([zeros, t, zeros]), dtype, lead, trail)
    s[:g] = float("nan")
    s[g + n:] = float("nan")
    return s[g:g + n]


@functools.lru_cache(maxsize=2)
def _device_operands(c):
    """x with GUARD lead channels, dy with 2 GUARD trail channels, y with both (inputs only: nothing writes them); 8 more channels behind x
    where two pixel strides would coincide."""
    from wu.layout import nhwc_ld
    x, dy, y = R.operands(c)
    dt = TORCH_DTYPE[c.dtype]
    extra = 8 if c.cin + GUARD in (c.cout + 2 * GUARD, c.cout + 3 * GUARD) else 0
    xd, dyd, yd = _put_guarded(x, dt, lead=GUARD, trail=extra), _put_guarded(dy, dt, trail=2 * GUARD), _put_guarded(y, dt, lead=GUARD, trail=2 * GUARD)
    lds = (nhwc_ld(xd), nhwc_ld(dyd), nhwc_ld(yd))
    assert len(set(lds)) == 3 and lds[0] > c.cin and min(lds[1:]) > c.cout, lds
    return xd, dyd, yd


def _gradients(c, with_db=True):
    """NaN-filled dw (Cout, Cin, 3, 3) and db (Cout,) inside NaN-filled flat buffers with GUARD floats on both sides."""
    dev = _dev()
    wbuf = torch.full((c.cout * c.cin * 9 + 2 * GUARD,), float("nan"), device=dev)
    bbuf = torch.full((c.cout + 2 * GUARD,), float("nan"), device=dev)
    return wbuf, wbuf[GUARD:-GUARD].view(c.cout, c.cin, 3, 3), bbuf, (bbuf[GUARD:-GUARD] if with_db else None)


def _launch(c, dy, y, act, dw, db, accumulate=False):
    from wu import kernels as K
    xd = _device_operands(c)[0]
    K.conv3x3_wgrad(xd, dy, dw, db, stride=c.stride, y=y, act=act if y is not None else R.NONE, accumulate=accumulate)


def _compare(got, want, name, what):
    """torch.equal against the oracle; a mismatch is reported by count, first index and tap."""
    if torch.equal(got, want):
        return
    bad = ((got != want) | torch.isnan(got)).nonzero()
    diff = (got - want).abs().nan_to_num(nan=float("inf")).max().item()
    taps = sorted({3 * int(i[2]) + int(i[3]) for i in bad.tolist()}) if got.dim() == 4 else []
    raise AssertionError(f"{what}: {name} differs from the CPU oracle in {len(bad)} of {got.numel()} elements, first index {bad[0].tolist()}, "
                         f"last {bad[-1].tolist()}, taps {taps}, {int(torch.isnan(got).sum())} NaN, max |diff| {diff}")


def _guards_intact(wbuf, bbuf, what):
    for buf in (wbuf, bbuf):
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), f"{what}: wrote outside its gradient"


def _premises(c):
    from wu import _lib
    p, r = R.check_features(c)
    assert int(_lib.load().wu_conv3x3_wgrad_workspace(c.n, c.h, c.w, c.cin, c.cout, c.stride, _code(c.dtype))) == p.ws == (p.splits * 9 * c.cout * c.cin + p.splits * c.cout) * 4
    if c.dtype == "bf16" and c.stride == 1:
        assert c.w % 32 != 0          # not a shape of the LDS-DMA kernel: the generic one runs
    return p, r


# ---------------------------------------------------------------------------------------------------------------------------------
# 3a: the four instances and the reducer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_conv3x3_wgrad_instances_are_exact(c):
    """conv3x3_wgrad_kernel<bf16_t,2,128>, <float,1,128>, <float,2,64> at tile widths 4, 8, 16, 32 and <bf16_t,1,256> at 4, 8, 16, with
    wgrad_reduce_kernel at wpr 1, 2, 4, 8 behind them: written into NaN (accumulate = 0), accumulated onto integers (accumulate = 1), and
    with db = None (the call of wu/resnet_train.py) -- each equals the CPU integer oracle bit for bit.  One pixel, one tile with one
    split (three of the reducer's four split groups read nothing), odd sizes at stride 2 (a last row and column without a partner),
    partial right tile columns and bottom tile rows, Cin != Cout, Cin = 192 and 512 (two trips of the reducer's column loop, the second
    with idle lanes), three to seven tiles per split in uneven walks, 480 splits."""
    p, r = _premises(c)
    _exact(R.bound(c))
    dev = _dev()
    _, dyd, _ = _device_operands(c)
    dw_ref, db_ref = (t.to(dev) for t in R.reference(c))
    what = f"{R.INSTANCE[(c.dtype, c.stride)]} {c.name} (TW {p.TW}, {p.ntiles} tiles on {p.splits} splits, wpr {r.wpr})"
    wbuf, dw, bbuf, db = _gradients(c)
    _launch(c, dyd, None, R.NONE, dw, db)
    _compare(dw, dw_ref, "dw", what)
    _compare(db, db_ref, "db", what)
    _guards_intact(wbuf, bbuf, what)
    dw0, db0 = R.ints(dw_ref.shape, -5, 5, 77).to(dev), R.ints(db_ref.shape, -5, 5, 78).to(dev)
    dw.copy_(dw0)
    db.copy_(db0)
    _launch(c, dyd, None, R.NONE, dw, db, accumulate=True)
    _compare(dw, dw0 + dw_ref, "dw", what + ", accumulate = 1")
    _compare(db, db0 + db_ref, "db", what + ", accumulate = 1")
    wbuf, dw, bbuf, _ = _gradients(c, with_db=False)
    _launch(c, dyd, None, R.NONE, dw, None)
    _compare(dw, dw_ref, "dw", what + ", db = None")
    _guards_intact(wbuf, bbuf, what + ", db = None")
    assert bool(torch.isnan(bbuf).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b: the in-kernel gate against the oracle (not against wu_act_gate)
# ---------------------------------------------------------------------------------------------------------------------------------
GATED = [(act, c) for act in (R.RELU, R.LEAKY) for c in R.gate_cases(act)]


@pytest.mark.parametrize("act,c", GATED, ids=lambda v: v.name if isinstance(v, R.WCase) else ACT_NAME[v])
def test_conv3x3_wgrad_in_kernel_gate_is_exact(act, c):
    """y != NULL: the staging loops of all four instances gate dy by the stored activation (gate16 in the stride-1 loop and in the
    stride-2 commit).  ReLU in both precisions; LeakyReLU in bf16, where the staged round_bf16(0.2f dy) is a multiple of 2^-10 and the
    sums stay exact (N Ho Wo < 8192) -- every tile width of every instance, against the oracle that gates on the CPU."""
    p, r = _premises(c)
    _exact(R.bound(c, act))
    dev = _dev()
    _, dyd, yd = _device_operands(c)
    dw_ref, db_ref = (t.to(dev) for t in R.reference(c, act))
    what = f"{R.INSTANCE[(c.dtype, c.stride)]} {c.name} gated in the kernel ({ACT_NAME[act]}, TW {p.TW})"
    wbuf, dw, bbuf, db = _gradients(c)
    _launch(c, dyd, yd, act, dw, db)
    _compare(dw, dw_ref, "dw", what)
    _compare(db, db_ref, "db", what)
    _guards_intact(wbuf, bbuf, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3c: LeakyReLU in fp32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.gate_cases(R.LEAKY, "fp32"), ids=lambda c: c.name)
def test_conv3x3_wgrad_fp32_leaky_gate(c):
    """conv3x3_wgrad_kernel<float,1,128> / <float,2,64> with a LeakyReLU gate.  Bitwise: the in-kernel gated run equals the same kernel fed
    the gradient pre-gated by wu_act_gate (same plan, same summation order, the same single multiply 0.2f g).  Bound: the pre-gated run
    lies within n_terms 2^-24 sum |x dy'| of the float64 result per element -- the forward error bound of an fp32 sum in any order, from
    the float64 oracle on |x|, |dy'|, not fitted to the kernel."""
    from wu import kernels as K
    _premises(c)
    dev = _dev()
    _, dyd, yd = _device_operands(c)
    what = f"{R.INSTANCE[(c.dtype, c.stride)]} {c.name} LeakyReLU"
    _, dw_a, _, db_a = _gradients(c)
    _launch(c, dyd, yd, R.LEAKY, dw_a, db_a)
    _, ho, wo = dyd.shape[1:]
    gbuf, gg = _sliced(c.n, c.cout, ho, wo, lead=0, trail=GUARD, dtype=torch.float32)
    K.act_gate(dyd, yd, R.LEAKY, out=gg)
    x, dy, y = R.operands(c)
    _check_slice(gbuf, c.cout, R.gated(dy, y, R.LEAKY, "fp32").to(dev), what + ": wu_act_gate", lead=0)
    _, dw_b, _, db_b = _gradients(c)
    _launch(c, gg, None, R.NONE, dw_b, db_b)
    _compare(dw_a, dw_b, "dw", what + ": gated in the kernel against pre-gated")
    _compare(db_a, db_b, "db", what + ": gated in the kernel against pre-gated")
    dw64, db64, bdw, bdb = R.error_bound(c, R.LEAKY)
    for name, got, want, bnd in (("dw", dw_b, dw64, bdw), ("db", db_b, db64, bdb)):
        assert not bool(torch.isnan(got).any())
        over = (got.double().cpu() - want).abs() - bnd
        assert float(over.max()) <= 0, f"{what}: {name} leaves the fp32 summation bound by {float(over.max())} (bound up to {float(bnd.max())})"


# ---------------------------------------------------------------------------------------------------------------------------------
# 3d: wu_act_gate alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [R.RELU, R.LEAKY], ids=["relu", "leaky"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_act_gate_is_exact(dtype, act):
    """act_gate_kernel<T, unsigned> (wu_act_gate) on its own against torch.where(y > 0, g, g.float() * 0.2f).to(dtype) -- one fp32
    multiply, one rounding: a few pixels, one 16-byte slot per pixel (C = 8 in bf16, 4 in fp32), more items than the largest grid has
    threads (the grid-stride loop turns); integer and non-integer gradients (0.2f g needs its rounding in bf16); g, y and out at three
    different pixel strides; out aliasing g.  The `long long` index instance needs more than 2^31 items: out of scope here."""
    from wu import kernels as K
    dt = TORCH_DTYPE[dtype]
    e = 8 if dtype == "bf16" else 4
    for si, shape in enumerate(R.ACT_GATE_SHAPES[dtype]):
        n, ch, h, w = shape
        big = n * h * w * ch // e > R.ACT_GATE_GRID_ITEMS
        assert big == (si == 2)
        for integers in ((False,) if big else (True, False)):
            g, y = R.act_gate_operands(shape, 7600 + si, integers)
            want = R.act_gate_reference(g, y, act, dt).to(_dev())
            for pg, py, po in (R.ACT_GATE_PADS[1:2] if big else R.ACT_GATE_PADS):
                what = f"wu_act_gate {dtype} {ACT_NAME[act]} {shape}, strides {ch + pg} / {ch + py} / {ch + po}, integers = {integers}"
                gd, yd = _put(g, dt, trail=pg), _put(y, dt, lead=py)
                buf, out = _sliced(n, ch, h, w, lead=0, trail=po, dtype=dt)
                K.act_gate(gd, yd, act, out=out)
                _check_slice(buf, ch, want, what, lead=0)
                assert torch.equal(gd.float().cpu(), g) and torch.equal(yd.float().cpu(), y), f"{what}: an input changed"
                K.act_gate(gd, yd, act, out=gd)          # out aliases g: every item reads its 16 bytes before it writes them
                assert torch.equal(gd, want), f"{what}: out aliasing g"


# ---------------------------------------------------------------------------------------------------------------------------------
# 3e: the y-gated scatter of wu_conv3x3_s2_dgrad
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.S2_GATE_CASES, ids=lambda c: c.name)
def test_s2_dgrad_gated_scatter_is_exact(c):
    """wu_conv3x3_s2_dgrad with y != NULL: upsample_zero_gate_kernel gates dy by the stored activation while it scatters it onto the even
    sites (the zero-stuffing path of a gradient that still needs its gate), then the stride-1 conv.  ReLU in both precisions, LeakyReLU
    in bf16, on two odd-sized shapes of _pointwise_ref.S2_CASES and one with more 16-byte items than the scatter's largest grid has
    threads.  Reference: the gate on the CPU (one multiply, one rounding), then s2_dgrad_reference; integer weights times multiples of
    2^-10, exact while 9 Cout |w| |dy'| 2^10 < 2^24 (asserted)."""
    from wu import kernels as K
    ops = R.s2_gate_operands(c)
    ho, wo = ops["dy"].shape[2:]
    for dtype, act in (("bf16", R.RELU), ("fp32", R.RELU), ("bf16", R.LEAKY)):
        _exact(R.s2_gate_bound(c, act))
        dt = TORCH_DTYPE[dtype]
        assert (c.n * c.h * c.w * c.cout // (8 if dtype == "bf16" else 4) > R.S2_UP_GRID_ITEMS) == (c is R.S2_GATE_CASES[2])
        _, wd = K.pack_conv3x3(ops["w"].to(_dev()), _code(dtype))
        dy, y = _put(ops["dy"], dt, trail=2 * GUARD), _put(ops["y"], dt, lead=GUARD, trail=2 * GUARD)
        lin, _ = PR.s2_dgrad_reference(c, dict(w=ops["w"], dy=R.gated(ops["dy"], ops["y"], act, dtype)), "ungated")
        assert int((ops["y"] == 0).sum()) > 0 and float(lin.abs().max()) > 0
        buf, dx = _sliced(c.n, c.cin, c.h, c.w, dtype=dt)
        K.conv3x3_s2_dgrad(dy, wd, dx, y=y, act=act)
        _check_slice(buf, c.cin, _rounded(lin, dt), f"wu_conv3x3_s2_dgrad gated by y ({ACT_NAME[act]}) {dtype} {c.name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3f: rejections
# ---------------------------------------------------------------------------------------------------------------------------------
def test_conv3x3_wgrad_rejects_bad_arguments():
    """wu_conv3x3_wgrad returns non-zero WITHOUT launching for stride 3, Cin = 96, ldx < Cin, a y whose pixel stride is no multiple of 16
    bytes and a workspace one byte short: dw and db are NaN before and after each call; the same call with the one argument put right
    succeeds and equals the oracle."""
    from wu import _lib
    from wu import kernels as K
    from wu.layout import nhwc_ld, stream_ptr
    c = next(c for c in R.CASES if (c.n, c.h, c.w, c.stride, c.dtype) == (2, 7, 7, 1, "bf16"))
    p, _ = _premises(c)
    xd, dyd, yd = _device_operands(c)
    ws = K.workspace(p.ws, _dev())
    wbuf, dw, bbuf, db = _gradients(c)
    good = dict(ldx=nhwc_ld(xd), y=None, ldy=0, act=R.NONE, ws_bytes=p.ws, cin=c.cin, stride=c.stride)

    def call(**kw):
        a = {**good, **kw}
        rc = _lib.load().wu_conv3x3_wgrad(xd.data_ptr(), a["ldx"], dyd.data_ptr(), nhwc_ld(dyd), a["y"], a["ldy"], a["act"], dw.data_ptr(), db.data_ptr(),
                                          ws.data_ptr(), a["ws_bytes"], c.n, c.h, c.w, a["cin"], c.cout, a["stride"], 0, _code(c.dtype), stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert (nhwc_ld(yd) + 4) * 2 % 16 != 0 and nhwc_ld(yd) + 4 >= c.cout and 56 * 2 % 16 == 0 and 56 < c.cin
    bad = {"stride = 3": dict(stride=3), "Cin = 96": dict(cin=96), "ldx < Cin": dict(ldx=56),
           "pixel stride of y off the 16-byte grid": dict(y=yd.data_ptr(), ldy=nhwc_ld(yd) + 4, act=R.RELU), "workspace one byte short": dict(ws_bytes=p.ws - 1)}
    for name, kw in bad.items():
        assert call(**kw) != 0, f"wu_conv3x3_wgrad accepted {name}"
        assert bool(torch.isnan(wbuf).all()) and bool(torch.isnan(bbuf).all()), f"wu_conv3x3_wgrad wrote a gradient although it refused {name}"
    assert call() == 0
    dw_ref, db_ref = (t.to(_dev()) for t in R.reference(c))
    _compare(dw, dw_ref, "dw", "the accepted call")
    _compare(db, db_ref, "db", "the accepted call")


def test_generic_plan_ignores_the_forced_grid():
    """The generic plan never reads option 10: its workspace (the split count) is the same on the whole chip and on a forced grid of 5,
    which is why this file forces no grid and takes its walks from shapes with more tiles than splits."""
    from wu import _lib
    c = next(c for c in R.CASES if c.n == 9)
    p, _ = R.plans(c)
    args = (c.n, c.h, c.w, c.cin, c.cout, c.stride, _code(c.dtype))
    assert int(_lib.load().wu_conv3x3_wgrad_workspace(*args)) == p.ws
    with _options({OPT_GRID: 5}):
        assert _cu_count() == 5
        assert int(_lib.load().wu_conv3x3_wgrad_workspace(*args)) == p.ws
    assert _cu_count() > 5
