"""The kernels of csrc/thin.hip -- the 3 -> 64 and 3 -> 3 image convs, their weight and data gradients, the 64 -> 3 tanh head --
against the EXACT CPU oracle of tests/_thin_ref.py, bit for bit, on every path the host dispatcher can take.

Operands are small integers (inv_sigma a power of two, gradients under a LeakyReLU gate multiples of 5), so every sum is an integer
below 2^24 and fp32 addition is exact in any order: the matrix-core, VALU, atomic and slab-fold paths must all give the oracle's bits
(tests/_thin_cases.py holds the tables and their bounds, tests/test_thin_ref_cpu.py checks both without a GPU).  The C ABI is driven
directly (wu.functional hides inv_sigma, accumulate and the workspace).  NHWC operands are the middle channel slice of a NaN-filled
wider buffer, NCHW outputs sit between NaN guards and start as NaN (accumulate = 0) or as integers (accumulate = 1).  Every comparison is
torch.equal on the device; the one exception is the tanh forward, compared with fp64 at the suite's 2e-5.

The prefetch loops of the matrix-core forward and weight gradient run a second iteration only above 524288 and 262144 output pixels (the
grid caps are hard-coded in thin.hip): the L shapes are the smallest that get there, as FULL and non-FULL instances, at both strides."""
import contextlib
import functools

import pytest
import torch

import _thin_cases as C
import _thin_ref as R
from _thin_ref import BF16, F32, LEAKY, NONE, RELU
from test_gpu_conv_walk import GUARD, _bits_buffer, _check_guards, _check_slice, _dev, _sliced

pytestmark = pytest.mark.gpu

OPT_C3_ROWS, OPT_IMG3_TILED = 5, 13                     # wu_set_option keys (csrc/wu_common.h)
DEFAULTS = {OPT_C3_ROWS: 0, OPT_IMG3_TILED: 1}          # the library's defaults (csrc/wu_prof.hip)
TDT = {BF16: torch.bfloat16, F32: torch.float32}
ACTS = (NONE, RELU, LEAKY)
NAN = float("nan")
_ids = lambda s: "x".join(str(v) for v in s)            # noqa: E731


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


def _call(name, *args):
    from wu import _lib
    from wu.layout import stream_ptr
    _lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream_ptr())


def _workspace():
    from wu import _lib, kernels as K
    return K.workspace(_lib.load().wu_thin_workspace_bytes(), _dev())


@functools.lru_cache(maxsize=None)
def _isg(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=_dev())


def _lead(ld):
    return {192: 64, 68: 2, 76: 8}[ld]


def _slice_of(t, dtype, ld=192):
    """CPU (N, C, H, W) integers -> a channel slice of a NaN-filled NHWC buffer with pixel stride ld (192: 64 channels in, 16-byte
    aligned; 68: 2 channels in, neither the address nor the stride aligned; 76: 8 channels in, an aligned address behind an unaligned
    stride).  Lossless: asserted."""
    n, c, h, w = t.shape
    lead = _lead(ld)
    _, sl = _sliced(n, c, h, w, lead, ld - lead - c, TDT[dtype])
    sl.copy_(t.to(_dev()))
    assert torch.equal(sl.float().cpu(), t) and sl.stride(3) == ld and sl.data_ptr() % 16 == (lead * sl.element_size()) % 16
    return sl


def _nchw(shape, init=None, off=0):
    """An fp32 NCHW tensor between NaN guards: NaN itself, or `init` (accumulate = 1).  off: floats by which its address misses 16-byte
    alignment."""
    numel = 1
    for v in shape:
        numel *= v
    flat = torch.full((numel + 2 * GUARD + off,), NAN, device=_dev())
    view = flat[GUARD + off:GUARD + off + numel].view(shape)
    assert view.data_ptr() % 16 == 4 * off
    if init is not None:
        view.copy_(init)
    return flat, view


def _same(got, want, what):
    """Bit for bit, no NaN left; the first differing index otherwise."""
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the CPU integer oracle; first index {idx[0].tolist()}, "
                             f"last {idx[-1].tolist()}; got {got[tuple(idx[0])].item()}, want {want[tuple(idx[0])].item()}")


def _check_nchw(flat, view, want, what, off=0):
    _same(view, want, what)
    assert bool(torch.isnan(flat[:GUARD + off]).all()) and bool(torch.isnan(flat[GUARD + off + view.numel():]).all()), f"{what}: wrote outside its tensor"


def _gate_ints(shape, seed):
    """A stored activation to gate by: integers with exact zeros ON the gate (y > 0 is false there)."""
    y = R.ints(shape, -2, 2, seed)
    assert int((y == 0).sum()) > 0 or y.numel() < 64
    return y


def _grad_ints(shape, seed, act):
    return R.ints(shape, -C.GMAX_LEAKY, C.GMAX_LEAKY, seed, 5) if act == LEAKY else R.ints(shape, -C.GMAX, C.GMAX, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 -> 64 forward
# ---------------------------------------------------------------------------------------------------------------------------------
def _fwd_operands(shape):
    n, h, w = shape
    R.exact(C.fwd_bound())
    return R.ints((n, 3, h, w), -C.XMAX, C.XMAX, 1), R.ints((64, 3, 3, 3), -C.WMAX, C.WMAX, 2), R.ints((64,), -C.BMAX, C.BMAX, 3)


def _bias_at(b, mod16):
    """The bias on the device at an address that is `mod16` past 16-byte alignment."""
    buf = torch.zeros((b.numel() + 4,), device=_dev())
    v = buf[mod16 // 4:mod16 // 4 + b.numel()]
    v.copy_(b)
    assert v.data_ptr() % 16 == mod16
    return v


def _run_fwd64(xd, wd, bd, isg, shape, stride, act, dtype, want, what, bits_want=None):
    n, h, w = shape
    ho, wo = R.out_hw(h, w, stride)
    buf, y = _sliced(n, 64, ho, wo, dtype=TDT[dtype])
    if bits_want is None:
        _call("wu_conv3x3_c3_fwd", xd, wd, bd, _isg(isg), y, 192, 0, n, h, w, 64, stride, act, dtype)
    else:
        from test_gpu_kernels import _decode_gate_bits
        assert act == RELU
        gbuf, gb = _bits_buffer(n, 64, ho, wo)
        _call("wu_conv3x3_c3_fwd_bits", xd, wd, bd, _isg(isg), y, 192, gb, n, h, w, 64, stride, dtype)
        assert torch.equal(_decode_gate_bits(gb, n, 64, ho, wo), bits_want), f"{what}: gate bits"
        _check_guards(gbuf, what)
    _check_slice(buf, 64, want, what)


def _want(y32, dtype):
    return (y32.bfloat16() if dtype == BF16 else y32).to(_dev())


@pytest.mark.parametrize("shape", C.E, ids=_ids)
def test_fwd64_edges(shape):
    """Every 3 -> 64 forward kernel on the edge set, both strides, all activations, with and without inv_sigma: the bf16 matrix-core
    kernel (plain and gate-bit entry), the VALU kernel (fp32; bf16 behind a bias that is not 16-byte aligned; WU_OPT_C3_ROWS = 2) and the
    rows kernel (WU_OPT_C3_ROWS = 1, both dtypes)."""
    x, wt, b = _fwd_operands(shape)
    xd, wd, bd, bd4 = x.to(_dev()), wt.to(_dev()), _bias_at(b, 0), _bias_at(b, 4)
    for stride in (1, 2):
        for isg in C.INV_SIGMAS:
            for act in ACTS:
                y32, bits = R.conv_fwd(x, wt, b, isg, stride, act)
                tag = f"{shape} stride {stride} act {act} inv_sigma {isg}"
                wb, wf = _want(y32, BF16), _want(y32, F32)
                _run_fwd64(xd, wd, bd, isg, shape, stride, act, BF16, wb, f"{tag} [mfma]")
                if act == RELU:
                    _run_fwd64(xd, wd, bd, isg, shape, stride, act, BF16, wb, f"{tag} [mfma, gate bits]", bits_want=bits)
                _run_fwd64(xd, wd, bd4, isg, shape, stride, act, BF16, wb, f"{tag} [bf16, bias + 4 bytes: VALU]")
                _run_fwd64(xd, wd, bd, isg, shape, stride, act, F32, wf, f"{tag} [fp32 VALU]")
                with _options({OPT_C3_ROWS: 1}):
                    _run_fwd64(xd, wd, bd, isg, shape, stride, act, BF16, wb, f"{tag} [rows bf16]")
                    _run_fwd64(xd, wd, bd, isg, shape, stride, act, F32, wf, f"{tag} [rows fp32]")
                with _options({OPT_C3_ROWS: 2}):
                    _run_fwd64(xd, wd, bd, isg, shape, stride, act, BF16, wb, f"{tag} [bf16 VALU by option]")
        # no bias at all (a NULL pointer is "aligned": the matrix-core kernel)
        y32, _ = R.conv_fwd(x, wt, None, None, stride, RELU)
        _run_fwd64(xd, wd, None, None, shape, stride, RELU, BF16, _want(y32, BF16), f"{shape} stride {stride} no bias [mfma]")


@functools.lru_cache(maxsize=None)
def _large(name):
    """Operands of an L shape on the device, once per module."""
    shape, stride = C.L[name]
    x, wt, b = _fwd_operands(shape)
    return x, wt, b, x.to(_dev()), wt.to(_dev()), _bias_at(b, 0)


@functools.lru_cache(maxsize=None)
def _large_ref(name, act, isg):
    """(bf16 output on the device, gate bits on the CPU) of an L shape, once per module."""
    shape, stride = C.L[name]
    x, wt, b = _large(name)[:3]
    y32, bits = R.conv_fwd(x, wt, b, isg, stride, act)
    return _want(y32, BF16), bits


@pytest.mark.parametrize("name,act,isg", [("L1", RELU, None), ("L1", NONE, 2.0), ("L2", RELU, 0.5), ("L2", NONE, None), ("L3", RELU, 2.0), ("L3", NONE, None),
                                          ("L4", RELU, None), ("L4", NONE, 0.5), ("L1x", NONE, None)])
def test_fwd64_mfma_more_than_one_iteration_per_wave(name, act, isg):
    """conv3x3_c3_fwd_mfma_kernel where its prefetch loop ITERATES (more than 4096 x 4 x 32 pixels): the patch requested one block
    ahead, the counted wait behind the stores, FULL (pixels % 32 == 0) and ragged instances, both strides, three iterations (L1x)."""
    shape, stride = C.L[name]
    assert C.npix(shape, stride) > R.FWD_MFMA_LOOP_PIXELS
    _, _, _, xd, wd, bd = _large(name)
    want, _ = _large_ref(name, act, isg)
    _run_fwd64(xd, wd, bd, isg, shape, stride, act, BF16, want, f"{name} {shape} stride {stride} act {act} inv_sigma {isg} [mfma]")


@pytest.mark.parametrize("name,isg", [("L1", None), ("L2", 0.5), ("L4", None)])
def test_fwd64_gate_bits_more_than_one_iteration_per_wave(name, isg):
    """The gate-bit instance against the ORACLE (not against the plain instance, which shares its loop): y, the bits, the guard words."""
    shape, stride = C.L[name]
    _, _, _, xd, wd, bd = _large(name)
    want, bits = _large_ref(name, RELU, isg)
    _run_fwd64(xd, wd, bd, isg, shape, stride, RELU, BF16, want, f"{name} {shape} [mfma, gate bits]", bits_want=bits)


def test_fwd64_rows_kernel_grid_stride_loop():
    """conv3x3_c3_fwd_rows_kernel on L2: 2068 blocks of 256 pixels over 2048 workgroups, the last block ragged."""
    shape, stride = C.L["L2"]
    assert C.npix(shape, stride) > R.ROWS_LOOP_PIXELS
    _, _, _, xd, wd, bd = _large("L2")
    want, _ = _large_ref("L2", RELU, 0.5)
    with _options({OPT_C3_ROWS: 1}):
        _run_fwd64(xd, wd, bd, 0.5, shape, stride, RELU, BF16, want, f"L2 {shape} [rows bf16]")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 -> 3 image conv, forward and data-gradient (FLIP) form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [1, 0], ids=["tiled", "per-pixel"])
@pytest.mark.parametrize("shape", C.IMG3_SHAPES, ids=_ids)
def test_img3_conv(shape, tiled):
    """img3_conv_kernel (WU_OPT_IMG3_TILED = 1) and the one-thread-per-pixel kernels behind option 0: forward with every activation and
    inv_sigma, the data gradient written and accumulated, and outputs whose base is 4-byte but not 16-byte aligned (W % 4 == 0: the
    scalar-store branch of the tiled kernel)."""
    n, h, w = shape
    dev = _dev()
    R.exact(C.fwd_bound())
    R.exact(C.dgrad_bound(3, C.GMAX))
    x = R.ints((n, 3, h, w), -C.XMAX, C.XMAX, 11)
    wt = R.ints((3, 3, 3, 3), -C.WMAX, C.WMAX, 12)
    b = R.ints((3,), -C.BMAX, C.BMAX, 13)
    dy = R.ints((n, 3, h, w), -C.GMAX, C.GMAX, 14)
    dx0 = R.ints((n, 3, h, w), -C.PRELOAD, C.PRELOAD, 15)
    xd, wd, bd, dyd = x.to(dev), wt.to(dev), b.to(dev), dy.to(dev)
    offs = (0, 1) if w % 4 == 0 else (0,)
    with _options({OPT_IMG3_TILED: tiled}):
        for isg in C.INV_SIGMAS:
            for off in offs:
                for act in ACTS:
                    y32, _ = R.conv_fwd(x, wt, b, isg, 1, act)
                    flat, y = _nchw((n, 3, h, w), off=off)
                    _call("wu_conv3x3_c3_fwd", xd, wd, bd, _isg(isg), y, 0, 1, n, h, w, 3, 1, act, F32)
                    _check_nchw(flat, y, y32.to(dev), f"{shape} tiled={tiled} forward act {act} inv_sigma {isg} offset {off}", off)
                ref = R.conv_dgrad(dy, None, NONE, wt, isg, 1, h, w).to(dev)
                for acc in (0, 1):
                    flat, dx = _nchw((n, 3, h, w), init=dx0 if acc else None, off=off)
                    _call("wu_conv3x3_c3_dgrad", dyd, 0, 1, None, 0, NONE, wd, _isg(isg), dx, n, h, w, 3, 1, acc, F32)
                    _check_nchw(flat, dx, ref + dx0.to(dev) if acc else ref, f"{shape} tiled={tiled} data gradient accumulate {acc} inv_sigma {isg} offset {off}", off)
        y32, _ = R.conv_fwd(x, wt, None, None, 1, NONE)
        flat, y = _nchw((n, 3, h, w))
        _call("wu_conv3x3_c3_fwd", xd, wd, None, None, y, 0, 1, n, h, w, 3, 1, NONE, F32)
        _check_nchw(flat, y, y32.to(dev), f"{shape} tiled={tiled} forward without bias")


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------
ALL_WAYS = [(True, 0, True), (False, 0, True), (True, 1, True), (False, 1, True), (True, 0, False), (False, 0, False), (True, 1, False)]
LARGE_WAYS = [(True, 0, True), (False, 0, True), (True, 1, True), (False, 1, False)]


def _run_wgrad(xd, dyd, lddy, nchw, yd, ldy, act, shape, cout, stride, dtype, dw_ref, db_ref, what, ways=ALL_WAYS):
    """(slab workspace or atomics, accumulate, with dbias): written into NaN, or added to integer-loaded gradients."""
    n, h, w = shape
    dev = _dev()
    ws = _workspace()
    dw0, db0 = R.ints(dw_ref.shape, -C.PRELOAD, C.PRELOAD, 77).to(dev), R.ints(db_ref.shape, -C.PRELOAD, C.PRELOAD, 78).to(dev)
    for slab, acc, with_db in ways:
        dw = dw0.clone() if acc else torch.full_like(dw0, NAN)
        db = (db0.clone() if acc else torch.full_like(db0, NAN)) if with_db else None
        _call("wu_conv3x3_c3_wgrad", xd, dyd, lddy, 1 if nchw else 0, yd, ldy, act, dw, db, ws if slab else None, ws.numel() if slab else 0,
              n, h, w, cout, stride, acc, dtype)
        tag = f"{what} [{'slab' if slab else 'atomics'}, accumulate {acc}, {'dbias' if with_db else 'no dbias'}]"
        _same(dw, dw0 + dw_ref if acc else dw_ref, f"{tag} dW")
        if with_db:
            _same(db, db0 + db_ref if acc else db_ref, f"{tag} db")


def _wgrad_case(shape, stride, dtype, nchw, cout, lddy, act, ways=ALL_WAYS, off=0):
    """One (shape, stride, layout, gate) case: operands, oracle, every way."""
    n, h, w = shape
    dev = _dev()
    ho, wo = R.out_hw(h, w, stride)
    gmax = C.GMAX_LEAKY if act == LEAKY else C.GMAX
    xm = C.wgrad_xmax(shape, stride, gmax)
    R.exact(C.wgrad_bound(shape, stride, gmax, xm))
    x = R.ints((n, 3, h, w), -xm, xm, 21)
    dy = _grad_ints((n, cout, ho, wo), 22, act)
    y = _gate_ints((n, cout, ho, wo), 23) if act != NONE else None
    dw_ref, db_ref = R.conv_wgrad(x, dy, y, act, stride)
    if nchw:
        _, dyd = _nchw(dy.shape, init=dy, off=off)
        yd = y.to(dev) if y is not None else None
        ld = 0
    else:
        dyd = _slice_of(dy, dtype, lddy)
        yd = _slice_of(y, dtype, lddy) if y is not None else None
        ld = lddy
    _run_wgrad(x.to(dev), dyd, ld, nchw, yd, ld, act, shape, cout, stride, dtype, dw_ref.to(dev), db_ref.to(dev),
               f"{shape} stride {stride} Cout {cout} gate {act} lddy {lddy} offset {off}", ways)


@pytest.mark.parametrize("shape", C.E, ids=_ids)
def test_wgrad_mfma_edges(shape):
    """conv3x3_c3_wgrad_mfma_kernel (bf16, NHWC dy): ungated and gated by ReLU / LeakyReLU in the kernel, both strides."""
    for stride in (1, 2):
        for act in ACTS:
            _wgrad_case(shape, stride, BF16, False, 64, 192, act)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", ["L1", "L2", "L4"])
def test_wgrad_mfma_several_tiles_per_workgroup(name, act):
    """... where its register prefetch ITERATES: 2 to 3 tiles of 256 pixels per workgroup, unevenly, a ragged last tile (L2, L4)."""
    shape, stride = C.L[name]
    assert C.npix(shape, stride) > 2 * R.WGRAD_MFMA_LOOP_PIXELS
    _wgrad_case(shape, stride, BF16, False, 64, 192, act, LARGE_WAYS)


@pytest.mark.parametrize("shape", C.WGRAD_GENERIC_SHAPES, ids=_ids)
def test_wgrad_generic(shape):
    """conv3x3_c3_wgrad_kernel: fp32 NHWC, and bf16 behind a dy whose pixel stride is not a multiple of 8 (the alignment fallback)."""
    ways = ALL_WAYS if C.npix(shape) < R.WGRAD_GENERIC_LOOP_PIXELS else LARGE_WAYS
    for stride in (1, 2):
        for act in ACTS:
            _wgrad_case(shape, stride, F32, False, 64, 192, act, ways)
            _wgrad_case(shape, stride, BF16, False, 64, 68, act, ways)
            if shape in C.E:
                _wgrad_case(shape, stride, BF16, False, 64, 76, act, LARGE_WAYS)


@pytest.mark.parametrize("shape", C.IMG3_WGRAD_SHAPES, ids=_ids)
def test_img3_wgrad(shape):
    """img3_wgrad_kernel: gated and ungated; 16-byte dy loads (W % 4 == 0, aligned base) and scalar ones (ragged W, or a base that is not
    16-byte aligned)."""
    large = shape[0] * -(-shape[1] // R.I3H) * -(-shape[2] // R.I3W) > R.IMG3_WGRAD_LOOP_TILES
    for act in ACTS:
        _wgrad_case(shape, 1, F32, True, 3, 0, act, LARGE_WAYS if large else ALL_WAYS)
        if shape[2] % 4 == 0 and not large:
            _wgrad_case(shape, 1, F32, True, 3, 0, act, LARGE_WAYS, off=1)


@pytest.mark.parametrize("shape", C.WGRAD_SMALL_SHAPES, ids=_ids)
def test_wgrad_small(shape):
    """conv3x3_c3_wgrad_small_kernel: the 3 -> 3 gradient with WU_OPT_IMG3_TILED = 0, stride 2, and Cout = 1 and 2."""
    ways = ALL_WAYS if C.npix(shape) < R.WGRAD_SMALL_LOOP_PIXELS else LARGE_WAYS
    for act in ACTS:
        with _options({OPT_IMG3_TILED: 0}):
            _wgrad_case(shape, 1, F32, True, 3, 0, act, ways)
        _wgrad_case(shape, 2, F32, True, 3, 0, act, ways)
    for cout in (1, 2):
        for stride in (1, 2):
            _wgrad_case(shape, stride, F32, True, cout, 0, RELU if cout == 1 else NONE, LARGE_WAYS)


# ---------------------------------------------------------------------------------------------------------------------------------
# data gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def _dgrad_case(shape, stride, dtype, nchw, cout, lddy, act, ldy=None, isgs=C.INV_SIGMAS):
    """One (shape, stride, layout, gate) case: written into NaN and accumulated onto integers, with and without inv_sigma."""
    n, h, w = shape
    dev = _dev()
    ho, wo = R.out_hw(h, w, stride)
    R.exact(C.dgrad_bound(cout, C.GMAX_LEAKY if act == LEAKY else C.GMAX))
    wt = R.ints((cout, 3, 3, 3), -C.WMAX, C.WMAX, 31)
    dy = _grad_ints((n, cout, ho, wo), 32, act)
    y = _gate_ints((n, cout, ho, wo), 33) if act != NONE else None
    dx0 = R.ints((n, 3, h, w), -C.PRELOAD, C.PRELOAD, 34)
    if nchw:
        dyd, yd, ld, ldyy = dy.to(dev), (y.to(dev) if y is not None else None), 0, 0
    else:
        ldyy = ldy or lddy
        dyd, yd, ld = _slice_of(dy, dtype, lddy), (_slice_of(y, dtype, ldyy) if y is not None else None), lddy
    wd = wt.to(dev)
    for isg in isgs:
        ref = R.conv_dgrad(dy, y, act, wt, isg, stride, h, w).to(dev)
        for acc in (0, 1):
            flat, dx = _nchw((n, 3, h, w), init=dx0 if acc else None)
            _call("wu_conv3x3_c3_dgrad", dyd, ld, 1 if nchw else 0, yd, ldyy, act, wd, _isg(isg), dx, n, h, w, cout, stride, acc, dtype)
            _check_nchw(flat, dx, ref + dx0.to(dev) if acc else ref,
                        f"{shape} stride {stride} Cout {cout} gate {act} lddy {lddy} ldy {ldyy} inv_sigma {isg} accumulate {acc}")


@pytest.mark.parametrize("shape", C.E, ids=_ids)
def test_dgrad_s2_mfma(shape):
    """conv3x3_c3_dgrad_s2_mfma_kernel: gated and ungated, with inv_sigma, written and accumulated."""
    for act in ACTS:
        _dgrad_case(shape, 2, BF16, False, 64, 192, act)


@pytest.mark.parametrize("shape", C.DGRAD_NHWC_SHAPES, ids=_ids)
def test_dgrad_nhwc(shape):
    """conv3x3_c3_dgrad_nhwc_kernel: bf16 stride 1, fp32 at both strides, bf16 stride 2 with 32 channels (with 64 aligned channels that
    call belongs to the matrix-core kernel)."""
    isgs = C.INV_SIGMAS if C.npix(shape) < 4096 * 16 else (2.0,)
    for act in ACTS:
        _dgrad_case(shape, 1, BF16, False, 64, 192, act, isgs=isgs)
        for stride in (1, 2):
            _dgrad_case(shape, stride, F32, False, 64, 192, act, isgs=isgs)
        if shape in C.E:
            _dgrad_case(shape, 2, BF16, False, 32, 192, act)


@pytest.mark.parametrize("shape", C.E, ids=_ids)
def test_dgrad_generic(shape):
    """conv3x3_c3_dgrad_kernel: NHWC behind an unaligned pixel stride; bf16 stride 2 behind a gate tensor that is not 16-byte aligned
    (it fails the alignment test of the matrix-core AND of the lane-group kernel, so the call falls through to here); NCHW gated with
    Cout = 3."""
    for act in ACTS:
        for stride in (1, 2):
            _dgrad_case(shape, stride, BF16, False, 64, 68, act)
            _dgrad_case(shape, stride, BF16, False, 64, 76, act, isgs=(0.5,))
            _dgrad_case(shape, stride, F32, True, 3, 0, act)
        if act != NONE:
            _dgrad_case(shape, 2, BF16, False, 64, 192, act, ldy=68)


def test_dgrad_generic_grid_stride_loop():
    """... on 8 x 520 x 512: 2.13 M input pixels on the 8192 x 256 grid."""
    shape = (8, 520, 512)
    assert C.npix(shape) > R.DGRAD_GENERIC_LOOP_PIXELS
    _dgrad_case(shape, 1, F32, True, 3, 0, RELU, isgs=(0.5,))


# ---------------------------------------------------------------------------------------------------------------------------------
# tanh head
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", C.HEAD_BWD_SHAPES, ids=_ids)
def test_head_bwd(shape, dtype):
    """wu_conv1x1_tanh_bwd, exact: out in {0, +-0.5} and dout a multiple of 4 make g = dout (1 - out^2) an integer.  x_gate_act none and
    ReLU (the fused graph's form), slab / atomics / accumulate, dx into a channel slice."""
    n, h, w = shape
    dev = _dev()
    R.exact(C.head_bwd_bound(shape))
    x = R.ints((n, 64, h, w), -C.XMAX, C.XMAX, 41)
    wt = R.ints((3, 64), -C.WMAX, C.WMAX, 42)
    dout = R.ints((n, 3, h, w), -8, 8, 43, 4)
    out = R.ints((n, 3, h, w), -1, 1, 44) * 0.5
    xd, wd, doutd, outd = _slice_of(x, dtype), wt.to(dev), dout.to(dev), out.to(dev)
    ws = _workspace()
    dw0, db0 = R.ints((3, 64), -C.PRELOAD, C.PRELOAD, 45).to(dev), R.ints((3,), -C.PRELOAD, C.PRELOAD, 46).to(dev)
    for gate in (NONE, RELU):
        dx_ref, dw_ref, db_ref = (t.to(dev) for t in R.tanh_head_bwd(dout, out, x, wt, gate))
        for slab, acc in ((True, 0), (False, 0), (True, 1), (False, 1)):
            buf, dx = _sliced(n, 64, h, w, dtype=TDT[dtype])
            dw = dw0.clone() if acc else torch.full_like(dw0, NAN)
            db = db0.clone() if acc else torch.full_like(db0, NAN)
            _call("wu_conv1x1_tanh_bwd", doutd, outd, xd, 192, wd, dx, 192, dw, db, ws if slab else None, ws.numel() if slab else 0,
                  n, h, w, 64, acc, gate, dtype)
            tag = f"{shape} dtype {dtype} x_gate_act {gate} [{'slab' if slab else 'atomics'}, accumulate {acc}]"
            _check_slice(buf, 64, dx_ref.to(TDT[dtype]), f"{tag} dx")
            _same(dw, dw0 + dw_ref if acc else dw_ref, f"{tag} dW")
            _same(db, db0 + db_ref if acc else db_ref, f"{tag} db")


_HEAD_FWD_WORST = {BF16: 0.0, F32: 0.0}


@pytest.mark.parametrize("dtype,cin", [(dt, c) for dt in (BF16, F32) for c in C.HEAD_FWD_CIN[dt]], ids=lambda v: str(v))
@pytest.mark.parametrize("shape", C.HEAD_FWD_SHAPES, ids=_ids)
def test_head_fwd(shape, dtype, cin):
    """wu_conv1x1_tanh_fwd against fp64 tanh(conv) on real inputs, every lane-group width (4, 8, 16, 64 lanes per pixel through the DPP
    mirrors and shuffles), x a channel slice; pre-activations of exactly +-40 give exactly +-1.  Bound: the suite's 2e-5
    (test_conv1x1_tanh); the kernel comment claims ~2e-7 and the largest error seen is printed, not asserted."""
    n, h, w = shape
    dev = _dev()
    g = torch.Generator().manual_seed(51)
    x = (torch.rand((n, cin, h, w), generator=g) * 2 - 1).to(TDT[dtype])
    wt = (torch.rand((3, cin), generator=g) * 2 - 1) * (2.0 / cin ** 0.5)
    b = torch.rand((3,), generator=g) - 0.5
    _, xd = _sliced(n, cin, h, w, dtype=TDT[dtype])
    xd.copy_(x.to(dev))
    flat, out = _nchw((n, 3, h, w))
    _call("wu_conv1x1_tanh_fwd", xd, xd.stride(3), wt.to(dev), b.to(dev), out, n, h, w, cin, dtype)
    assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + out.numel():]).all()) and not bool(torch.isnan(out).any())
    got = out.cpu().double()
    err = 0.0
    for i in range(0, n, 8):                 # fp64 reference in chunks of 8 images
        z = torch.einsum("nchw,kc->nkhw", x[i:i + 8].double(), wt.double()) + b.double().view(1, 3, 1, 1)
        err = max(err, (got[i:i + 8] - torch.tanh(z)).abs().max().item())
    _HEAD_FWD_WORST[dtype] = max(_HEAD_FWD_WORST[dtype], err)
    print(f"conv1x1_tanh_fwd {shape} dtype {dtype} Cin {cin}: max |err| vs fp64 {err:.3e}; largest so far bf16 {_HEAD_FWD_WORST[BF16]:.3e}, fp32 {_HEAD_FWD_WORST[F32]:.3e}")
    assert err <= 2e-5
    # saturation: x = 1, w = (+40 / Cin, -40 / Cin, 0), no offset: pre-activations are exactly +40, -40 and 0
    xd.fill_(1.0)
    ws = torch.stack([torch.full((cin,), 40.0 / cin), torch.full((cin,), -40.0 / cin), torch.zeros(cin)])
    flat, out = _nchw((n, 3, h, w))
    _call("wu_conv1x1_tanh_fwd", xd, xd.stride(3), ws.to(dev), torch.zeros(3, device=dev), out, n, h, w, cin, dtype)
    assert bool((out[:, 0] == 1.0).all()) and bool((out[:, 1] == -1.0).all()) and float(out[:, 2].abs().max()) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch is what the table says
# ---------------------------------------------------------------------------------------------------------------------------------
THIN_KERNELS = ["conv3x3_c3_fwd_mfma_kernel", "conv3x3_c3_fwd_rows_kernel", "conv3x3_c3_fwd_kernel", "img3_conv_kernel", "img3_wgrad_kernel",
                "conv3x3_c3_wgrad_mfma_kernel", "conv3x3_c3_wgrad_small_kernel", "conv3x3_c3_wgrad_kernel", "conv3x3_c3_dgrad_s2_mfma_kernel",
                "conv3x3_c3_dgrad_nhwc_kernel", "conv3x3_c3_dgrad_kernel", "conv1x1_tanh_fwd_kernel", "conv1x1_tanh_bwd_kernel"]


def _thin_kernels_of(fn):
    """The kernels of thin.hip the device ran during fn(), by name (torch.profiler sees every launch, whoever made it)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {k for k in THIN_KERNELS for nm in names if k in nm}, names         # no name in the list is a substring of another


def test_dispatch_reaches_the_kernel_the_table_names():
    """One representative call per kernel under torch.profiler: the device kernel's name is the one the dispatch restatement of
    tests/_thin_ref.py predicts for that call, and every kernel of the tables is reached."""
    dev = _dev()
    s = (2, 17, 19)
    n, h, w = s
    x, wt, b = _fwd_operands(s)
    xd, wd, bd, bd4 = x.to(dev), wt.to(dev), _bias_at(b, 0), _bias_at(b, 4)
    y1 = R.conv_fwd(x, wt, b, None, 1, RELU)[0]
    runs = []          # (predicted kernel, options, call)

    def fwd(dtype, bias, rows):
        return lambda: _run_fwd64(xd, wd, bias, None, s, 1, RELU, dtype, _want(y1, dtype), "dispatch")
    runs.append((R.fwd_kernel(BF16, False, n, h, w, 64, 1, 0), {}, fwd(BF16, bd, 0)))
    runs.append((R.fwd_kernel(BF16, False, n, h, w, 64, 1, 4), {}, fwd(BF16, bd4, 0)))
    runs.append((R.fwd_kernel(F32, False, n, h, w, 64, 1, 0), {}, fwd(F32, bd, 0)))
    runs.append((R.fwd_kernel(BF16, False, n, h, w, 64, 1, 0, c3_rows=1), {OPT_C3_ROWS: 1}, fwd(BF16, bd, 1)))
    runs.append((R.fwd_kernel(BF16, False, n, h, w, 64, 1, 0, c3_rows=2), {OPT_C3_ROWS: 2}, fwd(BF16, bd, 2)))
    for tiled in (1, 0):
        runs.append((R.fwd_kernel(F32, True, n, h, w, 3, 1, img3_tiled=tiled), {OPT_IMG3_TILED: tiled},
                     lambda: _call("wu_conv3x3_c3_fwd", xd, wd, None, None, _nchw((n, 3, h, w))[1], 0, 1, n, h, w, 3, 1, NONE, F32)))
        runs.append((R.dgrad_kernel(F32, True, n, h, w, 3, 1, img3_tiled=tiled), {OPT_IMG3_TILED: tiled}, lambda: _dgrad_case(s, 1, F32, True, 3, 0, NONE, isgs=(None,))))
        runs.append((R.wgrad_kernel(F32, True, n, h, w, 3, 1, img3_tiled=tiled), {OPT_IMG3_TILED: tiled}, lambda: _wgrad_case(s, 1, F32, True, 3, 0, NONE, LARGE_WAYS)))
    runs.append((R.wgrad_kernel(F32, True, n, h, w, 3, 2), {}, lambda: _wgrad_case(s, 2, F32, True, 3, 0, NONE, LARGE_WAYS)))
    runs.append((R.wgrad_kernel(BF16, False, n, h, w, 64, 1, 0, 192, 0, 192), {}, lambda: _wgrad_case(s, 1, BF16, False, 64, 192, RELU, LARGE_WAYS)))
    runs.append((R.wgrad_kernel(BF16, False, n, h, w, 64, 1, 4, 68, 4, 68), {}, lambda: _wgrad_case(s, 1, BF16, False, 64, 68, RELU, LARGE_WAYS)))
    runs.append((R.wgrad_kernel(F32, False, n, h, w, 64, 1, 0, 192, 0, 192), {}, lambda: _wgrad_case(s, 1, F32, False, 64, 192, RELU, LARGE_WAYS)))
    runs.append((R.dgrad_kernel(BF16, False, n, h, w, 64, 2, 0, 192, 0, 192), {}, lambda: _dgrad_case(s, 2, BF16, False, 64, 192, RELU, isgs=(None,))))
    runs.append((R.dgrad_kernel(BF16, False, n, h, w, 64, 1, 0, 192, 0, 192), {}, lambda: _dgrad_case(s, 1, BF16, False, 64, 192, RELU, isgs=(None,))))
    runs.append((R.dgrad_kernel(F32, False, n, h, w, 64, 2, 0, 192, 0, 192), {}, lambda: _dgrad_case(s, 2, F32, False, 64, 192, RELU, isgs=(None,))))
    runs.append((R.dgrad_kernel(BF16, False, n, h, w, 32, 2, 0, 192, 0, 192), {}, lambda: _dgrad_case(s, 2, BF16, False, 32, 192, RELU, isgs=(None,))))
    runs.append((R.dgrad_kernel(BF16, False, n, h, w, 64, 2, 0, 192, 4, 68), {}, lambda: _dgrad_case(s, 2, BF16, False, 64, 192, RELU, ldy=68, isgs=(None,))))
    runs.append((R.dgrad_kernel(BF16, False, n, h, w, 64, 1, 4, 68), {}, lambda: _dgrad_case(s, 1, BF16, False, 64, 68, NONE, isgs=(None,))))
    runs.append((R.dgrad_kernel(F32, True, n, h, w, 3, 1, 0, 0, 0, 0), {}, lambda: _dgrad_case(s, 1, F32, True, 3, 0, RELU, isgs=(None,))))
    runs.append(("conv1x1_tanh_bwd_kernel", {}, lambda: test_head_bwd((3, 5, 7), BF16)))
    runs.append(("conv1x1_tanh_fwd_kernel", {}, lambda: test_head_fwd((3, 5, 7), BF16, 64)))
    reached = set()
    for want, opts, fn in runs:
        with _options(opts):
            got, names = _thin_kernels_of(fn)
        assert got == {want}, f"predicted {want} (options {opts}), the device ran {sorted(got)}: {names}"
        reached |= got
    assert reached == set(THIN_KERNELS), f"never reached: {sorted(set(THIN_KERNELS) - reached)}"
