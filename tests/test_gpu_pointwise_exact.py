"""The estimator's pointwise GEMM family and stem (csrc/resnet.hip) against the EXACT CPU integer oracle of tests/_pointwise_ref.py:
conv1x1_mfma_kernel at its three tile heights, conv1x1_pw3_kernel pointwise and as the gathered 3 x 3 forms (with the kernels those
replace), conv1x1_chain_kernel, the four stem kernels.

Operands are small integers, so the fp32 sums are exact in any order and every kernel, tile, ring depth and path must produce the SAME
bits: torch's CPU fp32 result, with the kernels' epilogue order (bias, + residual, activation, gate, one rounding).  Every comparison is a
torch.equal.  tests/test_pointwise_ref_cpu.py proves for every case here that the bound holds, that fp32 equals float64, and that the
reference contains what makes a wrong kernel visible (values bf16 cannot hold, exact zeros on the activation and in the gate); the
cheap ones of these premises are asserted again next to the launch.  Outputs, residuals and gates are channel slices of wider NaN-filled
buffers; a forced grid (option 10) makes the persistent kernels WALK small shapes, and each such run asserts its items per workgroup."""
import contextlib
import functools

import pytest
import torch

import _pointwise_ref as R
from test_gpu_conv_walk import GUARD, _check_slice, _cu_count, _dev, _exact, _sliced

pytestmark = pytest.mark.gpu

# wu_set_option keys (csrc/wu_common.h) and the library's defaults (csrc/wu_prof.hip)
OPT_GRID, OPT_PW_TILE, OPT_S2_PARITY, OPT_PW3 = 10, 12, 14, 15
DEFAULTS = {OPT_GRID: 0, OPT_PW_TILE: 0, OPT_S2_PARITY: 1, OPT_PW3: 2 + 8 + (128 << 5)}
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32}


@contextlib.contextmanager
def _options(opts):
    """Set library options for the body; every one of them is back at its default afterwards, whatever happened."""
    from wu import _lib
    try:
        for k, v in opts.items():
            _lib.call("wu_set_option", k, v)
        yield
    finally:
        for k in opts:
            _lib.call("wu_set_option", k, DEFAULTS[k])


def _put(t, dtype, lead=0, trail=0):
    """CPU fp32 integers (N, C, H, W) -> the middle channel slice of a NaN-filled NHWC buffer of lead + C + trail channels (lossless: asserted)."""
    n, c, h, w = t.shape
    buf = torch.full((n, h, w, lead + c + trail), float("nan"), dtype=dtype, device=_dev()).permute(0, 3, 1, 2)
    s = buf[:, lead:lead + c]
    s.copy_(t.to(_dev()))
    assert torch.equal(s.float().cpu(), t)
    return s


def _rounded(v32, dtype):
    """The ONE rounding at the end of every epilogue (round to nearest even on both sides)."""
    return v32.to(dtype).to(_dev())


def _cheap_premises(lin, out, gate, bf16):
    assert int((lin == 0).sum()) > 0
    assert gate is None or int((gate == 0).sum()) > 0
    assert not bf16 or R.unrepresentable(out) >= 0.01


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the pointwise GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pw_reference(c):
    ops = R.pw_operands(c)
    lin, out = R.pw_reference(c, ops)
    _exact(R.pw_bound(c))
    _cheap_premises(lin, out, ops["gate"], c.dtype == "bf16")
    return ops, out


@functools.lru_cache(maxsize=8)
def _pw_device(c):
    """Device operands of a case (inputs only: nothing writes them)."""
    ops, _ = _pw_reference(c)
    dt = TORCH_DTYPE[c.dtype]
    return dict(x=_put(ops["x"], dt), w=ops["w"].to(_dev()).to(dt).contiguous(), bias=ops["bias"].to(_dev()) if ops["bias"] is not None else None,
                res=_put(ops["res"], dt, lead=GUARD) if ops["res"] is not None else None,
                gate=_put(ops["gate"], dt, trail=2 * GUARD) if ops["gate"] is not None else None)


def _run_pw(c, what):
    from wu import resnet as RN
    _, out = _pw_reference(c)
    d = _pw_device(c)
    dt = TORCH_DTYPE[c.dtype]
    _, _, act, gact = R.EPILOGUES[c.epi]
    buf, y = _sliced(c.n, c.cout, c.hout, c.wout, dtype=dt)
    RN.conv1x1(d["x"], d["w"], d["bias"], y, act=act, residual=d["res"], egate=d["gate"], egate_act=gact, in_stride=c.in_stride, out_stride=c.out_stride)
    _check_slice(buf, c.cout, _rounded(out, dt), what)


@pytest.mark.parametrize("c", R.PW_CASES, ids=lambda c: c.name)
def test_conv1x1_mfma_kernel_is_exact(c):
    """conv1x1_mfma_kernel itself (option 15 = 0), fp32 and bf16, as 64-, 128- and 256-row tiles (option 12 = 0, 2, 1): one to six K
    steps (every branch of the two-ahead pipeline), ragged last tiles, fewer rows than an MFMA block, 64 and 192 output channels, the six
    epilogues (LeakyReLU activation and gate among them), the stride-2 gather with odd and even inputs, the stride-2 scatter onto
    (2 Hc, 2 Wc), (2 Hc - 1, 2 Wc - 1) and (2 Hc, 2 Wc - 1) bare and with residual + gate -- every site of the NaN-filled output written."""
    with _options({OPT_PW3: 0, OPT_PW_TILE: R.TILE_OPTION[c.tile]}):
        _run_pw(c, f"conv1x1_mfma_kernel<{c.dtype}, {c.tile}> {c.name}")


@pytest.mark.parametrize("opt", R.PW3_OPTIONS, ids=lambda o: f"opt15={o}")
def test_conv1x1_pw3_kernel_pointwise_is_exact(opt):
    """conv1x1_pw3_kernel on the stride-1 bf16 cases above, against the oracle (not against the other kernel): ring depths 2-4, four and
    eight waves, the 64-cout tile (Cout = 64, 192) and the 128-cout tile, on the whole chip and on a forced grid of 3 CUs where every
    workgroup owns at least two items (asserted)."""
    walked, small = R.pw3_cases()
    for c in walked + small:
        with _options({OPT_PW3: opt}):
            _run_pw(c, f"conv1x1_pw3_kernel option 15 = {opt}, whole chip, {c.name}")
    for c in walked:
        with _options({OPT_PW3: opt, OPT_GRID: R.PW3_FORCED_CUS}):
            assert _cu_count() == R.PW3_FORCED_CUS
            items, grid = R.pw3_plan(c.n * c.hc * c.wc, c.cout, opt, _cu_count())
            assert items // grid >= 2, f"{c.name}: {items} items on {grid} workgroups"
            _run_pw(c, f"conv1x1_pw3_kernel option 15 = {opt}, {grid} workgroups x {items // grid}+ items, {c.name}")
    assert _cu_count() > R.PW3_FORCED_CUS          # options restored


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: the 3 x 3 stride-2 conv and its data gradient on every path
# ---------------------------------------------------------------------------------------------------------------------------------
def _forced(c, rows, couts, ncls, what):
    """The premise of a run on the forced grid: 2 x 3 workgroups at most; where the case is a walked one, at least two items each."""
    assert _cu_count() == R.S2_FORCED_CUS
    items, grid = R.pw3_conv_plan(rows, couts, ncls, _cu_count())
    assert grid == min(items, 2 * R.S2_FORCED_CUS)
    if c.walked:
        assert items // grid >= 2, f"{what}: {items} items on {grid} workgroups"


S2_FWD_PATHS = [("gathered rows", {OPT_PW3: R.S2_GATHERED}, False), ("gathered rows on 3 CUs", {OPT_PW3: R.S2_GATHERED, OPT_GRID: R.S2_FORCED_CUS}, True),
                ("register-staged", {OPT_PW3: 0}, False)]
S2_BWD_PATHS = [("gathered rows", {OPT_S2_PARITY: 1, OPT_PW3: R.S2_GATHERED}, False),
                ("gathered rows on 3 CUs", {OPT_S2_PARITY: 1, OPT_PW3: R.S2_GATHERED, OPT_GRID: R.S2_FORCED_CUS}, True),
                ("tap lists", {OPT_S2_PARITY: 1, OPT_PW3: 0}, False), ("zero stuffing", {OPT_S2_PARITY: 0, OPT_PW3: 0}, False)]


def _s2_setup(c, prec):
    from wu import _lib, kernels as K
    ops = R.s2_operands(c)
    for b in R.s2_bounds(c):
        _exact(b)
    dt = TORCH_DTYPE[prec]
    wf, wd = K.pack_conv3x3(ops["w"].to(_dev()), _lib.BF16 if prec == "bf16" else _lib.F32)
    return ops, dt, wf, wd


@pytest.mark.parametrize("c", R.S2_CASES, ids=lambda c: c.name)
def test_stride2_conv3x3_forward_every_path_is_exact(c):
    """Stride-2 3 x 3 forward (bias + LeakyReLU; bias + ReLU + output gate): conv1x1_pw3_kernel<.., CONV> on the whole chip and on 3 CUs and
    the register-staged kernel in bf16, the register-staged kernel in fp32.  The K orders differ, the integer oracle does not care: every
    path equals it, and therefore every other path."""
    from wu import kernels as K
    ho, wo = (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
    for prec in ("bf16", "fp32"):
        ops, dt, wf, _ = _s2_setup(c, prec)
        x, bias, gate = _put(ops["x"], dt), ops["bias"].to(_dev()), _put(ops["gate"], dt, trail=2 * GUARD)
        for epi, (act, gact) in R.S2_FWD_EPILOGUES.items():
            lin, out = R.s2_forward_reference(c, ops, epi)
            _cheap_premises(lin, out, ops["gate"] if gact != R.NONE else None, prec == "bf16")
            for label, opts, forced in S2_FWD_PATHS if prec == "bf16" else S2_FWD_PATHS[2:]:
                with _options(opts):
                    if forced:
                        _forced(c, c.n * ho * wo, c.cout, 1, f"{c.name} forward")
                    buf, y = _sliced(c.n, c.cout, ho, wo, dtype=dt)
                    K.conv3x3(x, wf, bias, y, 2, act, egate=gate if gact != R.NONE else None, egate_act=gact)
                    _check_slice(buf, c.cout, _rounded(out, dt), f"{c.name} {prec} forward {epi} [{label}]")
    assert _cu_count() > R.S2_FORCED_CUS


@pytest.mark.parametrize("epi", list(R.S2_DGRAD_EPILOGUES))
@pytest.mark.parametrize("c", R.S2_CASES, ids=lambda c: c.name)
def test_stride2_conv3x3_dgrad_every_path_is_exact(c, epi):
    """Data gradient of the stride-2 3 x 3 conv, ungated and LeakyReLU-gated: the four parity classes on conv1x1_pw3_kernel<.., CONV> (whole
    chip, 3 CUs), the parity tap lists on the register-staged kernel and zero stuffing in bf16; the latter two in fp32.  Every path is
    compared with the oracle (bias, + residual, activation, gate, then ONE rounding); all paths are run before the verdict.

    This test found the register-staged paths rounding a LeakyReLU-gated gradient TWICE (the gate's 0.2f applied to the stored bf16 value:
    28 of 512 elements of the 2 x 2 case, 41 510 of 362 496 of the 118 x 16 case, one ulp off, each equal to round(gate(round(dx)))) where
    the gathered-row form rounds once.  wu_conv3x3_s2_dgrad now gates the fp32 sum on every path (ConvArgs::late_gate, conv3x3_mfma.hip);
    the stride-1 data gradients of wu/disc_graph.py keep the two roundings of the stand-alone gate pass they replace.  A failure message
    still counts the elements that differ from that two-rounding value."""
    from wu import kernels as K
    gact = R.S2_DGRAD_EPILOGUES[epi]
    failures = []
    for prec in ("bf16", "fp32"):
        ops, dt, _, wd = _s2_setup(c, prec)
        dy, xgate = _put(ops["dy"], dt), _put(ops["xgate"], dt, lead=GUARD)
        lin, out = R.s2_dgrad_reference(c, ops, epi)
        _cheap_premises(lin, out, ops["xgate"] if gact != R.NONE else None, prec == "bf16")
        twice = _rounded(R.act_gate(lin.to(dt).float(), ops["xgate"], gact), dt)         # for the message only: gate applied to the ROUNDED gradient
        ho, wo = (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
        for label, opts, forced in S2_BWD_PATHS if prec == "bf16" else S2_BWD_PATHS[2:]:
            with _options(opts):
                if forced:
                    _forced(c, c.n * ho * wo, c.cin, 4, f"{c.name} data gradient")
                buf, dx = _sliced(c.n, c.cin, c.h, c.w, dtype=dt)
                K.conv3x3_s2_dgrad(dy, wd, dx, egate=xgate if gact != R.NONE else None, egate_act=gact)
                try:
                    _check_slice(buf, c.cin, _rounded(out, dt), f"{c.name} {prec} data gradient {epi} [{label}]")
                except AssertionError as e:
                    failures.append(f"{e} ({int((dx != twice).sum())} elements differ from round(gate(round(dx))))")
    assert _cu_count() > R.S2_FORCED_CUS
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: two chained GEMMs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CHAIN_CASES, ids=lambda c: c.name)
def test_conv1x1_chain_kernel_is_exact(c):
    """conv1x1_chain_kernel, forward form (bias + residual + ReLU, then bias + ReLU) and backward form (residual + gate, then gate): y1
    and y2 against the two-stage integer reference, whose second GEMM reads the ROUNDED y1 (a rounded integer is an integer)."""
    from wu import _lib, resnet as RN
    bf = torch.bfloat16
    ops = R.chain_operands(c)
    for b in R.chain_bounds(c):
        _exact(b)
    lin1, y1, lin2, y2 = R.chain_reference(c, ops)
    _cheap_premises(lin1, y1, ops["gate1"], True)
    _cheap_premises(lin2, y2, ops["gate2"], True)
    assert _lib.load().wu_conv1x1_chain_supported(c.k1, c.c1, c.c2, _lib.BF16)
    dev = _dev()
    x, res = _put(ops["x"], bf), _put(ops["res"], bf, lead=GUARD)
    wa, wb = RN.frag_pack(ops["wa"].to(dev).to(bf).contiguous()), RN.frag_pack(ops["wb"].to(dev).to(bf).contiguous())
    buf1, o1 = _sliced(1, c.c1, 1, c.m)
    buf2, o2 = _sliced(1, c.c2, 1, c.m)
    if c.form == "forward":
        RN.conv1x1_chain(x, wa, ops["bias_a"].to(dev), res, R.RELU, None, R.NONE, o1, wb, ops["bias_b"].to(dev), R.RELU, None, R.NONE, o2)
    else:
        g1, g2 = _put(ops["gate1"], bf, trail=2 * GUARD), _put(ops["gate2"], bf, lead=GUARD, trail=GUARD)
        RN.conv1x1_chain(x, wa, None, res, R.NONE, g1, R.RELU, o1, wb, None, R.NONE, g2, R.RELU, o2)
    _check_slice(buf1, c.c1, _rounded(y1, bf), f"conv1x1_chain_kernel {c.name}: y1")
    _check_slice(buf2, c.c2, _rounded(y2, bf), f"conv1x1_chain_kernel {c.name}: y2")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5, 6: the stem and its data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mfma", "valu_fp32", "valu_bf16"])
@pytest.mark.parametrize("c", R.STEM_FWD_CASES, ids=lambda c: c.name)
def test_stem_forward_is_exact(c, kind):
    """stem7x7_fwd_mfma_kernel (bf16; whole chip, and on one CU = two workgroups that walk at least three tiles each), the fp32 VALU kernel,
    and the bf16 VALU kernel that a bias pointer off the 16-byte grid selects: a one-tile image, tiles ragged in both directions, three
    tile columns; ReLU and no activation; the output is a 64-channel slice of a wider buffer."""
    from wu import _lib, resnet as RN
    dev = _dev()
    ops = R.stem_operands(c)
    _exact(R.stem_bounds()[0])
    lin, out = R.stem_forward_reference(c, ops)
    dt = torch.float32 if kind == "valu_fp32" else torch.bfloat16
    _cheap_premises(lin, out, None, dt == torch.bfloat16)
    x, w = ops["x"].to(dev).contiguous(), ops["w"].to(dev).contiguous()
    if kind == "valu_bf16":
        bias = torch.full((72,), float("nan"), device=dev)[1:65]
        bias.copy_(ops["bias"])
        assert bias.data_ptr() % 16 == 4
    else:
        bias = ops["bias"].to(dev)
        assert bias.data_ptr() % 16 == 0
    ho, wo = R.stem_out(c.h, c.w)
    want = _rounded(out, dt)
    code = _lib.F32 if kind == "valu_fp32" else _lib.BF16
    buf, y = _sliced(c.n, 64, ho, wo, dtype=dt)
    RN.stem7x7(x, w, bias, y, c.act, code)
    _check_slice(buf, 64, want, f"stem forward [{kind}] {c.name}")
    tiles = R.stem_fwd_tiles(c)
    if kind == "mfma" and tiles > c.n:          # a multi-tile image: walked by two workgroups
        with _options({OPT_GRID: 1}):
            assert _cu_count() == 1 and tiles // (2 * _cu_count()) >= 3, f"{tiles} tiles on two workgroups"
            buf, y = _sliced(c.n, 64, ho, wo, dtype=dt)
            RN.stem7x7(x, w, bias, y, c.act, code)
            _check_slice(buf, 64, want, f"stem forward [{kind}, two workgroups x {tiles // 2} tiles] {c.name}")
    assert _cu_count() > 1


@pytest.mark.parametrize("c", R.STEM_DGRAD_CASES, ids=lambda c: c.name)
def test_stem_dgrad_is_exact(c):
    """stem7x7_dgrad_mfma_kernel (bf16, even sizes; whole chip, and on one CU = two workgroups of at least three tiles each where the image
    has that many), the VALU kernel with bf16 gradients at odd sizes and with fp32 gradients: written into NaN, and accumulated onto
    integers; the images before and after the gradient stay untouched."""
    from wu import _lib, resnet as RN
    dev = _dev()
    ops = R.stem_dgrad_operands(c)
    _exact(R.stem_bounds()[1])
    ref = R.stem_dgrad_reference(c, ops).to(dev)
    dx0 = ops["dx0"].to(dev)
    dt, code = (torch.float32, _lib.F32) if c.kind == "fp32" else (torch.bfloat16, _lib.BF16)
    dy, w = _put(ops["dy"], dt), ops["w"].to(dev).contiguous()
    tiles = R.stem_dgrad_tiles(c)
    runs = [("whole chip", {})]
    if c.kind == "mfma" and tiles // 2 >= 3:
        runs.append(("two workgroups", {OPT_GRID: 1}))
    for label, opts in runs:
        with _options(opts):
            if opts:
                assert _cu_count() == 1 and tiles // (2 * _cu_count()) >= 3
            for accumulate in (False, True):
                full = torch.full((c.n + 2, 3, c.h, c.w), float("nan"), device=dev)
                dx = full[1:c.n + 1]
                if accumulate:
                    dx.copy_(dx0)
                RN.stem7x7_dgrad(dy, w, dx, code, accumulate=accumulate)
                want = dx0 + ref if accumulate else ref
                what = f"stem data gradient [{c.kind}, {label}, accumulate = {accumulate}] {c.name}"
                if not torch.equal(dx, want):
                    bad = ((dx != want) | torch.isnan(dx)).nonzero()
                    raise AssertionError(f"{what}: {len(bad)} of {dx.numel()} elements differ from the CPU integer oracle; first (n, c, h, w) = {bad[0].tolist()}, "
                                         f"last = {bad[-1].tolist()}; rows {int(bad[:, 2].min())}..{int(bad[:, 2].max())}, columns {int(bad[:, 3].min())}..{int(bad[:, 3].max())}")
                assert bool(torch.isnan(full[0]).all()) and bool(torch.isnan(full[c.n + 1]).all()), f"{what}: wrote outside its images"
    assert _cu_count() > 1
