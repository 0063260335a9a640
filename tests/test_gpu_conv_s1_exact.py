"""The register-staged template conv3x3_mfma_kernel<T, 1, MASKED> (csrc/conv3x3_mfma.hip) at stride 1, fp32 and bf16, and the small-image
kernel conv3x3_small_kernel<NHK, D> (csrc/conv3x3_small.hip) against the EXACT CPU integer oracle of tests/_conv_s1_ref.py.

Operands are small integers, so the fp32 sums are exact in any order and every tile width, chunk count, ring depth, K split and stacking
factor must produce the SAME bits: torch's CPU fp32 result with the kernels' epilogue order (bias, activation, one rounding; an output gate
on the STORED value, rounded again).  Every comparison is a torch.equal.  tests/test_conv_s1_ref_cpu.py proves for every case here that the
bound holds, that fp32 equals float64, that the reference contains what makes a wrong kernel visible, and -- from the plan restatements
template_plan / small_plan -- which tile width, chunk count, template instance, ring depth and stacking factor each case reaches.  Every
operand (x, mask, gate) and every output is the middle channel slice of a NaN-filled buffer: a read of a neighbouring channel poisons the
result, a write outside the slice is caught.  The one combination without an exact oracle (a leaky input mask in fp32) stays with
tests/test_gpu_kernels.py::test_conv3x3_gated_abi_paths."""
import contextlib
import functools

import pytest
import torch

import _conv_s1_ref as R
from test_gpu_conv_walk import GUARD, _check_slice, _cu_count, _dev, _exact, _sliced
from test_gpu_pointwise_exact import TORCH_DTYPE, _put, _rounded

pytestmark = pytest.mark.gpu

DEFAULTS = dict(R.DEFAULTS)          # options 0 (LDS-DMA conv), 3 (small-image kernel), 10 (forced CU count) and the library's defaults
KERNELS = ("conv3x3_mfma_kernel", "conv3x3_small_kernel", "conv3x3_mfma_v2_kernel")      # no name is a substring of another
DISPATCH_KERNEL = {"template": KERNELS[0], "small": KERNELS[1], "v2": KERNELS[2]}


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


def _small_supported(n, h, w, cin, cout):
    from wu import _lib
    return bool(_lib.load().wu_conv3x3_small_supported(n, h, w, cin, cout, cout, cin, cout))


def _assert_defaults():
    """Options 0, 3 and 10 are at their defaults, read back through the library's own predicates (it has no getter): the whole chip; the
    LDS-DMA conv on; the small-image kernel on (an 8 x 8 image is taken) and subject to its dispatch rule (a full chip of 16 x 16 images is not)."""
    from wu import _lib
    cus = _cu_count()
    assert cus > 16
    assert _lib.load().wu_conv3x3_gate_bits_supported(32, 32, 64, 64, 64, 64, _lib.BF16) == 1
    assert _small_supported(1, 8, 8, 64, 64) and not _small_supported(*R.rule_probes(cus)[0])


@functools.lru_cache(maxsize=None)
def _reference(c):
    """(operands, fp32 value in front of the last rounding) of a case, computed once on the CPU; the cheap premises next to it."""
    ops = R.s1_operands(c)
    _exact(R.s1_bound(c))
    lin, pre, out = R.s1_reference(c, ops)
    _, act, gact, mact, _ = R.EPILOGUES[c.epi]
    assert act == R.NONE or int((lin == 0).sum()) > 0
    assert gact == R.NONE or int((ops["gate"] == 0).sum()) > 0
    assert mact == R.NONE or int((ops["mask"] == 0).sum()) > 0
    assert c.dtype != "bf16" or R.unrepresentable(pre) >= 0.01
    return ops, out


def _device(c):
    """Device operands: x, mask and gate as channel slices of NaN-filled buffers (NaN channels on both sides of x, in front of the mask, behind
    the gate: three different pixel strides), and the weight pack the case reads (the rotated one for the data-gradient form)."""
    from wu import _lib, kernels as K
    ops, _ = _reference(c)
    dt = TORCH_DTYPE[c.dtype]
    dgrad = R.EPILOGUES[c.epi][4]
    packs = K.pack_conv3x3(ops["w"].to(_dev()), _lib.BF16 if c.dtype == "bf16" else _lib.F32)
    return dict(x=_put(ops["x"], dt, lead=GUARD, trail=GUARD), w=packs[1] if dgrad else packs[0],
                bias=ops["bias"].to(_dev()) if ops["bias"] is not None else None,
                mask=_put(ops["mask"], dt, lead=GUARD) if ops["mask"] is not None else None,
                gate=_put(ops["gate"], dt, trail=2 * GUARD) if ops["gate"] is not None else None)


def _conv3x3(c, d):
    """One wu_conv3x3_fwd call of the case into a fresh NaN-filled slice."""
    from wu import kernels as K
    _, act, gact, mact, _ = R.EPILOGUES[c.epi]
    buf, y = _sliced(c.n, c.cout, c.h, c.w, dtype=TORCH_DTYPE[c.dtype])
    K.conv3x3(d["x"], d["w"], d["bias"], y, 1, act, mask=d["mask"], mask_act=mact, egate=d["gate"], egate_act=gact)
    return buf


def _predicted(c, opts):
    has_b, act, gact, mact, _ = R.EPILOGUES[c.epi]
    return R.dispatch(c.dtype, c.n, c.h, c.w, c.cin, c.cout, has_b, act, gact != R.NONE, mact != R.NONE, opts, _cu_count())


@pytest.mark.parametrize("c", R.TEMPLATE_CASES, ids=lambda c: c.name)
def test_conv3x3_template_stride1_is_exact(c):
    """conv3x3_mfma_kernel<float | bf16, 1, MASKED> through wu_conv3x3_fwd: tiles 4, 8, 16 and 32 pixels wide, two tile rows and a ragged
    last row and column at every width, 2 x 2 and 3 x 2 tiles, one full tile; one, two, three and four K chunks (no / one / several
    store_chunk inside the loop); one and three cout tiles; N = 1, 2, 3; bias, bias + ReLU, bias + LeakyReLU, the data-gradient form on the
    rotated pack with a ReLU and a leaky output gate, bias + ReLU + gate, a ReLU input mask, a leaky input mask in bf16.  In bf16 every
    route that ends at the template is taken: Cin = 32, a gate with a bias on a shape of the LDS-DMA conv, option 0 = 0, option 3 = 0, a mask."""
    _, out = _reference(c)
    d = _device(c)
    opts = R.ROUTES[c.route]
    with _options(opts):
        assert _predicted(c, opts) == "template"
        buf = _conv3x3(c, d)
        p = R.template_plan(c.h, c.w, c.cin, c.dtype)
        _check_slice(buf, c.cout, _rounded(out, TORCH_DTYPE[c.dtype]),
                     f"conv3x3_mfma_kernel<{c.dtype}, 1> {c.name} ({p.tiles_y} x {p.tiles_x} tiles of {p.TH} x {1 << p.tw_log2}, {p.nchunks} chunks)")
    _assert_defaults()


@pytest.mark.parametrize("c", R.SMALL_CASES, ids=lambda c: c.name)
def test_conv3x3_small_is_exact(c):
    """conv3x3_small_kernel<3, 3>, <4, 3> and <5, 2>: tiles 4, 8 and 16 pixels wide; one, two and three row tiles of one image; two, four,
    six, eight, thirteen and seventeen stacked images per tile, with a partly empty last group, unused tile rows and the 320-pixel cap; one,
    two, three, four and eight chunks at ring depth 3 and one, two and three at depth 2; bias + ReLU, bias + LeakyReLU, nothing, and the
    data-gradient form with a ReLU and a leaky gate.  Each case runs through wu_conv3x3_fwd with the kernel forced (option 3 = 2, the
    library's pack), through wu_conv3x3_small_fwd (chunk-major weights), and through wu_conv3x3_fwd with the kernel switched off (option 3
    = 0: the template on the same shape).  All three equal the oracle, hence each other; all three run before the verdict."""
    from wu import kernels as K
    _, out = _reference(c)
    d = _device(c)
    _, act, gact, _, _ = R.EPILOGUES[c.epi]
    want = _rounded(out, torch.bfloat16)
    p = R.small_plan(c.n, c.h, c.w, c.cin, c.cout)
    assert p is not None and p.nhk <= R.SMALL_MAX_NHK
    nhk, depth = R.small_instance(p)
    tag = f"{c.name} ({p.ipt} images x {p.tiles_y} x {p.tiles_x} tiles {1 << p.tw_log2} wide, {p.nchunks} chunks, {p.groups} groups)"
    runs = []
    with _options({R.OPT_CONV_SMALL: 2}):
        assert K.conv3x3_small_supported(d["x"], c.cout), "shape outside conv3x3_small_kernel"
        assert _predicted(c, {R.OPT_CONV_SMALL: 2}) == "small"
        runs.append((f"conv3x3_small_kernel<{nhk}, {depth}> forced, library pack", _conv3x3(c, d)))
    buf, y = _sliced(c.n, c.cout, c.h, c.w)
    K.conv3x3_small(d["x"], K.chunk_major(d["w"]), d["bias"], y, act, egate=d["gate"], egate_act=gact)
    runs.append((f"conv3x3_small_kernel<{nhk}, {depth}> chunk-major weights", buf))
    with _options({R.OPT_CONV_SMALL: 0}):
        assert _predicted(c, {R.OPT_CONV_SMALL: 0}) == "template"
        runs.append(("conv3x3_mfma_kernel<bf16, 1> (option 3 = 0)", _conv3x3(c, d)))
    failures = []
    for label, buf in runs:
        try:
            _check_slice(buf, c.cout, want, f"{label}: {tag}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    _assert_defaults()


def test_small_dispatch_rule():
    """wu_conv3x3_small_supported (what wu_conv3x3_fwd itself asks) against the restatement of tests/_conv_s1_ref.py: a batch of 16 x 16 images
    on each side of N * 4 >= 3 * CUs, an 8-wide image the rule never sends away; on the whole chip and with the CU count held at 8; with the
    kernel forced (the rule is skipped) and switched off.  The predicate only: nothing is launched at these batch sizes."""
    def check(cus, opt3):
        assert _cu_count() == cus
        probes = R.rule_probes(cus)
        want = [R.small_preferred(*s, cus, opt3) for s in probes]
        assert [_small_supported(*s) for s in probes] == want, (cus, opt3, probes)
        return want

    cus = _cu_count()
    assert check(cus, 1) == [False, True, True]
    with _options({R.OPT_GRID: 8}):
        assert check(8, 1) == [False, True, True]
        assert R.rule_probes(8)[0][0] == 6
    with _options({R.OPT_CONV_SMALL: 2}):
        assert check(cus, 2) == [True, True, True]
    with _options({R.OPT_CONV_SMALL: 0}):
        assert check(cus, 0) == [False, False, False]
    # shapes the kernel itself declines, whatever the rule: too wide, Cin off the 32-channel chunk, Cout off the 64-channel tile
    for s in ((1, 8, 17, 64, 64), (1, 8, 8, 48, 64), (1, 8, 8, 64, 32)):
        assert R.small_plan(*s) is None and not _small_supported(*s)
    _assert_defaults()


def _kernels_of(fn):
    """(the conv kernels of KERNELS the device ran during fn(), every device kernel name): torch.profiler sees every launch."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {k for k in KERNELS for nm in names if k in nm}, names


def test_dispatch_reaches_the_kernel_the_plan_names():
    """One representative call per route under torch.profiler: the template for fp32 and for each of the five bf16 routes, the small-image
    kernel for the forced and the chunk-major run, the LDS-DMA conv for a plain W > 16 call at default options (the control: the very case
    that option 0 = 0 sends to the template)."""
    from wu import kernels as K
    for k in KERNELS:
        assert not any(k in other for other in KERNELS if other != k)
    runs = []          # (label, options, case, call or None for wu_conv3x3_fwd)
    for route, opts in R.ROUTES.items():
        c = next(c for c in R.TEMPLATE_CASES if c.route == route)
        runs.append((f"route {route}", opts, c, None))
    control = next(c for c in R.TEMPLATE_CASES if c.route == "opt0")
    runs.append(("control: default options", {}, control, None))
    small = R.SMALL_CASES[1]
    runs.append(("small forced", {R.OPT_CONV_SMALL: 2}, small, None))
    runs.append(("small at default options", {}, small, None))

    def chunk_major(c, d):
        _, act, gact, _, _ = R.EPILOGUES[c.epi]
        K.conv3x3_small(d["x"], K.chunk_major(d["w"]), d["bias"], _sliced(c.n, c.cout, c.h, c.w)[1], act, egate=d["gate"], egate_act=gact)

    runs.append(("small, chunk-major weights", {}, small, chunk_major))
    reached = set()
    for label, opts, c, call in runs:
        d = _device(c)
        torch.cuda.synchronize()
        with _options(opts):
            want = "small" if call is not None else _predicted(c, opts)
            got, names = _kernels_of((lambda: call(c, d)) if call is not None else (lambda: _conv3x3(c, d)))
        assert got == {DISPATCH_KERNEL[want]}, f"{label}, {c.name}: predicted {DISPATCH_KERNEL[want]}, the device ran {sorted(got)}: {names}"
        if label.startswith("route"):
            assert want == "template", label
        reached |= got
    assert reached == set(KERNELS)
    _assert_defaults()
