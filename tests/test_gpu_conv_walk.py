"""The persistent tile walk of conv3x3_mfma_v2_kernel and the tile loop of conv3x3_wgrad_v2_kernel against an EXACT CPU reference.

A persistent workgroup carries state from one tile to the next (one-tile-ahead fetch descriptors and border-lane masks, the previous tile's
packed outputs / gate words / head pixels stored from inside the next tile's first chunk, counted waits that depend on which of those stores
are in flight, the LDS-resident weight slab, the final flush).  None of that runs when a workgroup owns one tile, which is what every small
shape gives on a whole chip.  Here `wu_set_option(10, g)` holds the grid at g workgroups, so that small shapes are WALKED, and every case
asserts that premise (tiles per workgroup, tiles per split) instead of trusting a comment.

The oracle is exact: operands are small integers.  bf16 holds integers up to 256 exactly, a product of two bf16 values is exact in fp32,
and an fp32 sum of integers is exact in ANY order while it stays below 2^24 -- so whatever the tiling, chunk order, split-K fold or MFMA
shape, the kernels and torch's CPU fp32 convolution must agree bit for bit (`_exact` asserts the bound for each case).  bf16 outputs are
compared with `ref.bfloat16()` (round to nearest even on both sides; sums above 256 exercise the rounding), fp32 outputs with `ref`.
Exact zeros sit on the ReLU gate (y > 0) and 2x2 windows tie (first maximum in scan order), both on purpose."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# wu_set_option keys (csrc/wu_common.h) and the library's defaults (csrc/wu_prof.hip)
OPT_CONV_V2, OPT_PERSISTENT, OPT_WGRAD_V2, OPT_WGRAD_DMA_INTERLEAVE, OPT_STRIDED, OPT_GRID, OPT_W_RESIDENT = 0, 1, 2, 4, 7, 10, 11
DEFAULTS = {OPT_CONV_V2: 1, OPT_PERSISTENT: 1, OPT_WGRAD_V2: 1, OPT_WGRAD_DMA_INTERLEAVE: 1, OPT_STRIDED: 1, OPT_GRID: 0, OPT_W_RESIDENT: 1}
BITS_SENTINEL = 0x55555555
GUARD = 64           # sentinel words / channels on both sides of an output


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


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


def _cu_count():
    from wu import _lib
    return int(_lib.load().wu_cu_count())


def _ints(shape, lo, hi, seed):
    """Seeded integers in [lo, hi] as fp32 (exact in bf16)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def _exact(bound):
    """The premise of the oracle: every partial sum is an integer below 2^24, so fp32 addition is exact in any order."""
    assert bound < 2 ** 24, f"integer oracle out of range: worst-case sum {bound} >= 2^24"


def _bf16_dev(t):
    """CPU fp32 integers (N, C, H, W) -> NHWC bf16 on the GPU (lossless: asserted)."""
    assert float(t.abs().max()) <= 256
    return t.to(_dev()).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _sliced(n, c, h, w, lead=GUARD, trail=GUARD, dtype=torch.bfloat16):
    """A NaN-filled NHWC buffer of lead + c + trail channels and its middle channel slice (the zero-copy concat form)."""
    buf = torch.full((n, h, w, lead + c + trail), float("nan"), dtype=dtype, device=_dev()).permute(0, 3, 1, 2)
    return buf, buf[:, lead:lead + c]


def _check_slice(buf, c, want, what, lead=GUARD):
    """The middle slice equals `want` bit for bit (no NaN left, nothing wrong), the neighbouring channels are untouched."""
    got = buf[:, lead:lead + c]
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the CPU integer oracle; first (n, c, h, w) = "
                             f"{idx[0].tolist()}, last = {idx[-1].tolist()}; images {sorted(set(idx[:, 0].tolist()))}, "
                             f"rows {int(idx[:, 2].min())}..{int(idx[:, 2].max())}, columns {int(idx[:, 3].min())}..{int(idx[:, 3].max())}")
    assert bool(torch.isnan(buf[:, :lead]).all()) and bool(torch.isnan(buf[:, lead + c:]).all()), f"{what}: wrote outside its channel slice"


def _bits_buffer(n, c, h, w):
    """A sentinel-filled gate-bit buffer (uint32 [N*H*W][C/64][2], include/wu_kernels.h) with guard words on both sides."""
    words = n * h * w * (c // 64) * 2
    buf = torch.full((words + 2 * GUARD,), BITS_SENTINEL, dtype=torch.int32, device=_dev())
    return buf, buf[GUARD:GUARD + words]


def _check_guards(buf, what):
    assert bool((buf[:GUARD] == BITS_SENTINEL).all()) and bool((buf[-GUARD:] == BITS_SENTINEL).all()), f"{what}: wrote outside the bit plane"


def _decode_bits(bits, n, c, h, w):
    """uint32 [N*H*W][C/64][2] -> bool (N, C, H, W): bit 8k + i of word (pixel, ct, hf) is channel 64 ct + 16 k + 8 hf + i."""
    dev = bits.device
    wv = bits.view(n, h, w, c // 64, 1, 2, 1).to(torch.int64) & 0xffffffff
    sh = (8 * torch.arange(4, device=dev).view(4, 1, 1) + torch.arange(8, device=dev).view(1, 1, 8))
    return ((wv >> sh) & 1).bool().reshape(n, h, w, c).permute(0, 3, 1, 2)


def _encode_bits(pos):
    """bool (N, C, H, W) -> the int32 words `_decode_bits` reads."""
    n, c, h, w = pos.shape
    dev = pos.device
    p = pos.permute(0, 2, 3, 1).reshape(n, h, w, c // 64, 4, 2, 8).to(torch.int64)
    sh = (8 * torch.arange(4, device=dev).view(4, 1, 1) + torch.arange(8, device=dev).view(1, 1, 8))
    word = (p << sh).sum(dim=(-3, -1))
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32).reshape(-1).contiguous()


def _pool_reference(y):
    """(2x2 max-pool of the stored bf16 y, "this element is its window's first maximum in scan order") from torch's CPU max_pool2d."""
    n, c, h, w = y.shape
    pooled, idx = F.max_pool2d(y.float().cpu(), 2, return_indices=True)
    sel = torch.zeros((n, c, h * w), dtype=torch.bool).scatter_(2, idx.reshape(n, c, -1), True).view(n, c, h, w)
    return pooled.bfloat16().to(y.device), sel.to(y.device)


def test_bit_plane_helpers_agree_with_the_suite_decoder():
    """This file's GPU-side encoder / decoder against the decoder test_gpu_kernels.py uses (written from the same header text)."""
    from test_gpu_kernels import _decode_gate_bits
    g = torch.Generator().manual_seed(5)
    pos = torch.rand((2, 128, 3, 5), generator=g) > 0.5
    words = _encode_bits(pos.to(_dev()))
    assert torch.equal(_decode_gate_bits(words, 2, 128, 3, 5), pos)
    assert torch.equal(_decode_bits(words, 2, 128, 3, 5).cpu(), pos)


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk of conv3x3_mfma_v2_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
TH, TW = 16, 32       # the kernel's pixel tile (csrc/conv3x3_mfma_v2.hip, struct K); a tile is TH x TW pixels x 64 output channels


def _tile_dims(shape):
    n, cin, cout, h, w = shape
    return n, -(-h // TH), -(-w // TW), cout // 64


def _ntiles(shape):
    n, ty, tx, ct = _tile_dims(shape)
    return n * ty * tx * ct


def _walks(ntiles, grid, strided):
    """The tile ids each persistent workgroup visits, in order (conv3x3_mfma_v2_kernel: t_begin / t_end / t_step)."""
    if strided:
        return [list(range(wg, ntiles, grid)) for wg in range(grid)]
    return [list(range(ntiles * wg // grid, ntiles * (wg + 1) // grid)) for wg in range(grid)]


def _decode_tile(shape, t):
    """tile id -> (n, ty, tx, ct): cout tile fastest, then tile column, tile row, image."""
    _, tiles_y, tiles_x, cts = _tile_dims(shape)
    ct, t = t % cts, t // cts
    tx, t = t % tiles_x, t // tiles_x
    return t // tiles_y, t % tiles_y, tx, ct


def _walk_features(shape, grid, strided):
    """What the walks of this (shape, grid) contain; each case names the features it is there for and they are asserted."""
    n, cin, cout, h, w = shape
    _, tiles_y, tiles_x, _ = _tile_dims(shape)
    feats = set()

    def edge(t):          # the fetch masks lanes at the top / left / right border; bottom rows fall off the image descriptor
        _, ty, tx, _ = t
        return ty == 0 or tx == 0 or ty == tiles_y - 1 or tx == tiles_x - 1

    def partial(t):       # a tile that is not `ov_interior`: some lanes store nothing, the wait after it is not the counted one
        _, ty, tx, _ = t
        return (ty + 1) * TH > h or (tx + 1) * TW > w

    for walk in _walks(_ntiles(shape), grid, strided):
        ts = [_decode_tile(shape, t) for t in walk]
        for a, b in zip(ts, ts[1:]):
            if a[0] != b[0]:
                feats.add("wraps_image")
            if a[0] == b[0] and a[1] != b[1]:
                feats.add("wraps_row")
            if a[:3] == b[:3] and a[3] != b[3]:
                feats.add("consecutive_cout_tiles")
        for a, b, c in zip(ts, ts[1:], ts[2:]):
            if edge(a) and not edge(b) and edge(c):
                feats.add("edge_inner_edge")
            if partial(a) and not partial(b) and partial(c):
                feats.add("partial_full_partial")
            if not partial(a) and partial(b) and not partial(c):
                feats.add("full_partial_full")
    return feats


# (N, Cin, Cout, H, W), forced grid, features the strided / the contiguous walk must show.  Grids of 5 and 7 divide no tile count below,
# so contiguous ranges are uneven and strided walks wrap tile rows and images at varying places.
WALK_CASES = [
    # half-empty right column only (W = 56); Cin = 64 with ONE cout tile: the weight slab stays in LDS; odd N
    ((3, 64, 64, 48, 56), 5, {"wraps_row", "wraps_image", "full_partial_full"}, {"wraps_row", "wraps_image"}),
    # half-empty right column only (W = 112), four tile columns; Cin = 64 with TWO cout tiles: weights re-fetched per tile; N = 1
    ((1, 64, 128, 32, 112), 5, {"wraps_row"}, {"wraps_row", "consecutive_cout_tiles"}),
    # half-empty bottom row only (H = 24)
    ((3, 64, 64, 24, 96), 5, {"wraps_row", "wraps_image"}, {"wraps_row", "wraps_image"}),
    # half-empty bottom row only (H = 40), three tile columns and rows; Cin = 192: six chunks per tile, 8 waves by default
    ((2, 192, 64, 40, 96), 5, {"wraps_row", "wraps_image", "partial_full_partial"}, {"wraps_row", "wraps_image", "edge_inner_edge"}),
    # ragged in both directions; Cin = 256: eight chunks, 4 waves by default; two cout tiles
    ((2, 256, 128, 40, 72), 7, {"wraps_row", "wraps_image"}, {"wraps_row", "wraps_image", "consecutive_cout_tiles"}),
    # a single, partial tile column (W = 24) and a half-empty bottom row; odd N
    ((3, 64, 128, 40, 24), 5, {"wraps_row", "wraps_image"}, {"wraps_row", "wraps_image", "consecutive_cout_tiles"}),
    # Cin = 768: 24 chunks per tile, 4 waves by default; four cout tiles; N = 1
    ((1, 768, 256, 24, 56), 5, {"wraps_row"}, {"wraps_row", "consecutive_cout_tiles"}),
    # NOT ragged, 4 x 4 tiles: border tile -> interior tile -> border tile in one workgroup (every tile is a full one: the counted waits)
    ((2, 64, 64, 64, 128), 5, {"wraps_row", "wraps_image", "edge_inner_edge"}, {"wraps_row", "wraps_image"}),
    # odd N, ragged both ways, 3 x 3 tiles of which the middle one is the only full interior tile; Cin = 128, two cout tiles
    ((3, 128, 128, 40, 72), 7, {"wraps_row", "wraps_image", "partial_full_partial"}, {"wraps_row", "wraps_image", "consecutive_cout_tiles"}),
]


def _walk_configs(shape, grid):
    """(label, options, forced grid or None) of every run of one shape: both wave counts x (one tile per workgroup, strided walk,
    contiguous walk), and the non-resident weight path where the resident one exists (Cin == 64, one cout tile, 8 waves)."""
    n, cin, cout, h, w = shape
    out = []
    for waves, mode in ((4, 2), (8, 3)):
        walks = [("one tile per workgroup", {OPT_PERSISTENT: 0}, None),
                 ("strided walk", {OPT_GRID: grid, OPT_STRIDED: 1}, grid),
                 ("contiguous walk", {OPT_GRID: grid, OPT_STRIDED: 0}, grid)]
        for label, opts, g in walks:
            out.append((f"{waves} waves, {label}", {**opts, OPT_CONV_V2: mode}, g, waves))
            if waves == 8 and cin == 64 and cout == 64:
                out.append((f"{waves} waves, {label}, weights not resident", {**opts, OPT_CONV_V2: mode, OPT_W_RESIDENT: 0}, g, waves))
    return out


def _assert_walk_premise(shape, g):
    """The grid really is g workgroups and every one of them walks a first, a middle and a last tile."""
    assert _cu_count() == g, f"forced grid not in effect: wu_cu_count() = {_cu_count()}, wanted {g}"
    nt = _ntiles(shape)
    assert nt % g != 0 and nt // g >= 3, f"{nt} tiles on {g} workgroups: fewer than 3 tiles per workgroup, or an even split"
    for strided in (True, False):
        assert min(len(wk) for wk in _walks(nt, g, strided)) >= 3


@pytest.mark.parametrize("case", WALK_CASES, ids=lambda c: "x".join(str(v) for v in c[0]) + f"-g{c[1]}")
def test_conv3x3_v2_tile_walk_is_exact(case):
    """Every epilogue instance of conv3x3_mfma_v2_kernel (GATED 0..5) at both wave counts, as one tile per workgroup, as a strided walk and
    as a contiguous walk on a forced small grid, with resident and re-fetched weights: every run equals the CPU integer oracle bit for bit
    (and hence every other run).  Outputs, pooled tensors and the head image start as NaN, bit planes as 0x55555555 with guard words, and
    every 64-channel-multiple output is a channel slice of a wider buffer whose other channels must stay NaN."""
    from wu import kernels as K
    shape, grid, want_strided, want_contig = case
    n, cin, cout, h, w = shape
    dev = _dev()
    assert want_strided <= _walk_features(shape, grid, True), (want_strided, _walk_features(shape, grid, True))
    assert want_contig <= _walk_features(shape, grid, False), (want_contig, _walk_features(shape, grid, False))

    # ---- operands and the CPU reference (fp32 on integers: exact) ----
    _exact(9 * max(cin, cout) * 2 * 1 + 3)
    x = _ints((n, cin, h, w), -2, 2, 100)
    wt = _ints((cout, cin, 3, 3), -1, 1, 101)
    bias = _ints((cout,), -3, 3, 102)
    pre = F.conv2d(x, wt, bias, padding=1)
    assert int((pre == 0).sum()) > 0, "no exact zero on the ReLU gate"
    y_none, y_relu = pre.bfloat16().to(dev), F.relu(pre).bfloat16().to(dev)
    pooled, sel = _pool_reference(y_relu)
    # the data-gradient form: this kernel shape (Cin -> Cout) is the data gradient of a forward conv Cout -> Cin with weight wg
    wg = _ints((cin, cout, 3, 3), -1, 1, 103)
    egate = _ints((n, cout, h, w), -2, 2, 104)
    dgrad = torch.nn.grad.conv2d_input((n, cout, h, w), wg, x, padding=1)
    d_gated = (dgrad * (egate > 0)).bfloat16().to(dev)
    assert int((egate == 0).sum()) > 0

    xd, bd, ed = _bf16_dev(x), bias.to(dev), _bf16_dev(egate)
    wf, _ = K.pack_conv3x3(wt.to(dev), K._lib.BF16)
    _, wd = K.pack_conv3x3(wg.to(dev), K._lib.BF16)
    ebits = _encode_bits(ed.float() > 0)
    probe = _sliced(n, cout, h, w)[1]
    assert K.gate_bits_supported(xd, probe), "shape outside conv3x3_mfma_v2_kernel"
    head = cout == 64 and cin < 256          # the shapes of GATED == 5 (8 waves, one cout tile)
    if head:
        assert K.conv3x3_head_supported(xd)
        g = torch.Generator().manual_seed(105)
        # |y| runs to a few hundred here: head weights small enough that tanh is not saturated (|z| of order 1)
        hw_ = ((torch.rand((3, 64), generator=g) * 2 - 1) * 0.006).to(dev)
        hb = ((torch.rand((3,), generator=g) * 2 - 1) * 0.3).to(dev)
        z = torch.einsum("kc,nchw->nkhw", hw_.double().cpu(), y_relu.double().cpu()) + hb.double().cpu().view(1, 3, 1, 1)
        head_want = torch.tanh(z)
        assert float((head_want.abs() < 0.9).double().mean()) > 0.5, "head reference saturated"
    head_ref = None

    for label, opts, g, waves in _walk_configs(shape, grid):
        with _options(opts):
            if g is not None:
                _assert_walk_premise(shape, g)
            tag = f"{shape} [{label}]"
            # GATED 0: plain forward, no activation and ReLU
            for act, want in ((K.ACT_NONE, y_none), (K.ACT_RELU, y_relu)):
                buf, y = _sliced(n, cout, h, w)
                K.conv3x3(xd, wf, bd, y, 1, act)
                _check_slice(buf, cout, want, f"{tag} forward act={act}")
            # GATED 1: data-gradient form gated by a tensor
            buf, y = _sliced(n, cout, h, w)
            K.conv3x3(xd, wd, None, y, 1, K.ACT_NONE, egate=ed, egate_act=K.ACT_RELU)
            _check_slice(buf, cout, d_gated, f"{tag} data gradient, gate tensor")
            # GATED 2: ... gated by bits
            buf, y = _sliced(n, cout, h, w)
            K.conv3x3_bits(xd, wd, None, y, K.ACT_NONE, egate_bits=ebits)
            _check_slice(buf, cout, d_gated, f"{tag} data gradient, gate bits")
            # GATED 3: forward + ReLU + gate bits
            buf, y = _sliced(n, cout, h, w)
            gbuf, gb = _bits_buffer(n, cout, h, w)
            K.conv3x3_bits(xd, wf, bd, y, K.ACT_RELU, gate_bits_out=gb)
            _check_slice(buf, cout, y_relu, f"{tag} forward + gate bits")
            assert torch.equal(_decode_bits(gb, n, cout, h, w), y_relu > 0), f"{tag}: gate bits"
            _check_guards(gbuf, f"{tag} gate bits")
            # GATED 0 + pool
            buf, y = _sliced(n, cout, h, w)
            pbuf, pool = _sliced(n, cout, h // 2, w // 2)
            K.conv3x3_relu_pool(xd, wf, bd, y, pool)
            _check_slice(buf, cout, y_relu, f"{tag} forward + pool")
            _check_slice(pbuf, cout, pooled, f"{tag} pooled tensor")
            # GATED 4: + pool + gate / arg-max bits
            buf, y = _sliced(n, cout, h, w)
            pbuf, pool = _sliced(n, cout, h // 2, w // 2)
            gbuf, gb = _bits_buffer(n, cout, h, w)
            sbuf, sb = _bits_buffer(n, cout, h, w)
            K.conv3x3_relu_pool_bits(xd, wf, bd, y, pool, gb, sb)
            _check_slice(buf, cout, y_relu, f"{tag} forward + pool + bits")
            _check_slice(pbuf, cout, pooled, f"{tag} pooled tensor (+ bits)")
            assert torch.equal(_decode_bits(gb, n, cout, h, w), y_relu > 0), f"{tag}: gate bits (pool instance)"
            assert torch.equal(_decode_bits(sb, n, cout, h, w), sel), f"{tag}: arg-max bits"
            _check_guards(gbuf, f"{tag} gate bits (pool instance)")
            _check_guards(sbuf, f"{tag} arg-max bits")
            # GATED 5 (8 waves only): + the 64 -> 3 head and tanh; the 64-channel output is exact, the image keeps the float64 comparison
            if head and waves == 8:
                buf, y = _sliced(n, cout, h, w)
                out = torch.full((n + 2, 3, h, w), float("nan"), device=dev)
                K.conv3x3_relu_head(xd, wf, bd, y, hw_, hb, out[1:n + 1])
                out2 = torch.full((n + 2, 3, h, w), float("nan"), device=dev)
                K.conv3x3_relu_head(xd, wf, bd, None, hw_, hb, out2[1:n + 1])
                _check_slice(buf, cout, y_relu, f"{tag} forward + head")
                for o in (out, out2):
                    assert bool(torch.isnan(o[0]).all()) and bool(torch.isnan(o[n + 1]).all()), f"{tag}: head wrote outside its image"
                    assert not bool(torch.isnan(o[1:n + 1]).any()), f"{tag}: head pixels missing"
                err = (out[1:n + 1].double().cpu() - head_want).abs().max().item()
                assert err < 2e-6, f"{tag}: head vs float64 {err}"
                assert torch.equal(out[1:n + 1], out2[1:n + 1]), f"{tag}: head without y differs"
                if head_ref is None:
                    head_ref = out[1:n + 1].clone()
                assert torch.equal(out[1:n + 1], head_ref), f"{tag}: head image differs between walks"
    assert _cu_count() > grid        # options restored


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile loop of conv3x3_wgrad_v2_kernel, and the generic weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad_v2_eligible(h, w, cin, cout):
    """csrc/conv3x3_wgrad_v2.hip, wgrad_v2_eligible, for bf16 / stride 1 / an ungated gradient."""
    return w % 32 == 0 and cin % 64 == 0 and cout % 64 == 0


def _wgrad_v2_plan(n, h, w, cin, cout, cus):
    """csrc/conv3x3_wgrad_v2.hip, wgrad_v2_plan: 8 x 32-pixel tiles, one split per (CUs / channel blocks), at most one per tile."""
    ntiles = n * (w // 32) * -(-h // 8)
    blocks = (cin // 64) * (cout // 64)
    splits = min(max(1, cus // blocks), ntiles)
    tiles_per_split = -(-ntiles // splits)
    return ntiles, -(-ntiles // tiles_per_split), tiles_per_split


def _wgrad_reference(shape, seed, gated=False):
    n, cin, cout, h, w = shape
    _exact(n * h * w * 2 * 1 + 8)
    x = _ints((n, cin, h, w), -2, 2, seed)
    gy = _ints((n, cout, h, w), -1, 1, seed + 1)
    y = _ints((n, cout, h, w), -2, 2, seed + 2) if gated else None
    g_eff = gy * (y > 0) if gated else gy
    dw = torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), g_eff, padding=1)
    db = g_eff.sum(dim=(0, 2, 3))
    return x, gy, y, dw, db


def _run_wgrad(xd, gyd, yd, dw_ref, db_ref, what):
    """accumulate = 0 into NaN-filled gradients, then accumulate = 1 on top of integer-loaded ones: both exact."""
    from wu import kernels as K
    dev = _dev()
    cout, cin = dw_ref.shape[:2]
    kw = dict(y=yd, act=K.ACT_RELU) if yd is not None else {}
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=dev)
    db = torch.full((cout,), float("nan"), device=dev)
    K.conv3x3_wgrad(xd, gyd, dw, db, **kw)
    for name, got, want in (("dw", dw, dw_ref), ("db", db, db_ref)):
        if not torch.equal(got, want):
            d = (got - want)
            bad = (got != want).nonzero()
            raise AssertionError(f"{what}: {name} differs from the CPU integer oracle in {len(bad)} of {got.numel()} elements, first index "
                                 f"{bad[0].tolist()}, max |diff| {d.abs().nan_to_num(nan=float('inf')).max().item()}")
    dw0, db0 = _ints(dw_ref.shape, -5, 5, 77).to(dev), _ints(db_ref.shape, -5, 5, 78).to(dev)
    dw, db = dw0.clone(), db0.clone()
    K.conv3x3_wgrad(xd, gyd, dw, db, accumulate=True, **kw)
    assert torch.equal(dw, dw0 + dw_ref) and torch.equal(db, db0 + db_ref), f"{what}: accumulate = 1"


# (N, Cin, Cout, H, W), (forced grid, splits it must give, uneven last split), ...
WGRAD_V2_CASES = [
    # W = 32: one tile column, left AND right padding flags on the same tile; H = 36: five tile rows, the last half empty; 25 tiles
    ((5, 64, 64, 36, 32), [(1, 1, False), (2, 2, True), (3, 3, True)]),
    # W = 96: an interior tile column; two channel blocks; H = 20: a half-empty bottom row; 27 tiles
    ((3, 128, 64, 20, 96), [(2, 1, False), (4, 2, True), (6, 3, False)]),
    # three channel blocks on the output side; H = 12; 12 tiles
    ((3, 64, 192, 12, 64), [(3, 1, False), (6, 2, False), (9, 3, False)]),
    # more channel blocks (6) than workgroups (4): the split count clamps to 1 and one workgroup per block walks all 12 tiles
    ((2, 192, 128, 24, 64), [(4, 1, False)]),
]


@pytest.mark.parametrize("case", WGRAD_V2_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_conv3x3_wgrad_v2_tile_loop_is_exact(case):
    """conv3x3_wgrad_v2_kernel with several tiles per split (forced grids giving 1, 2 and 3 splits, an uneven last split), on the whole
    chip (one tile per split), as 8 and as 4 waves, with and without the interleaved DMA issue: dw and db equal the CPU integer oracle bit
    for bit, written and accumulated."""
    shape, grids = case
    n, cin, cout, h, w = shape
    assert _wgrad_v2_eligible(h, w, cin, cout)
    x, gy, _, dw_ref, db_ref = _wgrad_reference(shape, 200)
    dev = _dev()
    xd, gyd, dw_ref, db_ref = _bf16_dev(x), _bf16_dev(gy), dw_ref.to(dev), db_ref.to(dev)
    _run_wgrad(xd, gyd, None, dw_ref, db_ref, f"{shape} whole chip")
    for g, want_splits, uneven in grids:
        for label, extra in (("8 waves", {}), ("4 waves", {OPT_WGRAD_V2: 2}), ("8 waves, DMA issue not interleaved", {OPT_WGRAD_DMA_INTERLEAVE: 0})):
            with _options({**extra, OPT_GRID: g}):
                assert _cu_count() == g
                ntiles, splits, tps = _wgrad_v2_plan(n, h, w, cin, cout, _cu_count())
                assert splits == want_splits and tps >= 3, f"{shape} on {g} workgroups: {splits} splits of {tps} tiles"
                assert (ntiles % tps != 0) == uneven
                _run_wgrad(xd, gyd, None, dw_ref, db_ref, f"{shape} on {g} workgroups ({splits} splits x {tps} tiles, {label})")
    for label, extra in (("4 waves", {OPT_WGRAD_V2: 2}), ("DMA issue not interleaved", {OPT_WGRAD_DMA_INTERLEAVE: 0})):
        with _options(extra):
            _run_wgrad(xd, gyd, None, dw_ref, db_ref, f"{shape} whole chip, {label}")
    assert _cu_count() > 9


@pytest.mark.parametrize("shape", [(3, 64, 128, 40, 72), (2, 128, 64, 28, 56), (1, 64, 64, 33, 35)])
@pytest.mark.parametrize("gated", [False, True])
def test_conv3x3_wgrad_generic_is_exact(shape, gated):
    """The generic weight gradient (W % 32 != 0, or gated in the kernel by the stored activation y): the path of ten of the thirteen
    weight gradients at 224 x 224.  Run twice, the second time with option 10 = 5: the generic plan never reads that option (its split
    count is ceil(512 / channel blocks) capped by the tile count), so the second run repeats the first -- it shows that a forced grid
    changes nothing here, it is NOT a walk.  All three shapes give one tile per split (asserted from the plan mirror in
    tests/test_wgrad_ref_cpu.py).  The tile loop of conv3x3_wgrad_kernel<bf16_t,1,256> is walked by test_unet_layers_at_224_are_exact
    (512 -> 512 at 28 x 28: 8 tiles per split), that of the other three instances by the 45 x 79 cases of tests/test_gpu_wgrad_exact.py
    (3 to 7 tiles per split, uneven)."""
    n, cin, cout, h, w = shape
    assert gated or not _wgrad_v2_eligible(h, w, cin, cout)
    x, gy, y, dw_ref, db_ref = _wgrad_reference(shape, 300, gated)
    dev = _dev()
    xd, gyd, yd = _bf16_dev(x), _bf16_dev(gy), (_bf16_dev(y) if gated else None)
    dw_ref, db_ref = dw_ref.to(dev), db_ref.to(dev)
    _run_wgrad(xd, gyd, yd, dw_ref, db_ref, f"{shape} generic, gated={gated}, whole chip")
    with _options({OPT_GRID: 5}):
        assert _cu_count() == 5
        _run_wgrad(xd, gyd, yd, dw_ref, db_ref, f"{shape} generic, gated={gated}, 5 workgroups")


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's default training shape: 224 x 224, B = 16 (t_cls_train.py:20,24), whole chip, default options
# ---------------------------------------------------------------------------------------------------------------------------------
# (Cin, Cout, H = W, batch, position in r_double_conv, forward form in wu/unet_graph.py).  Widths 112 / 56 / 28 give a half-empty right
# tile column, heights 56 / 28 a half-empty bottom row.  Batch 16 throughout, as the reference trains (the CPU reference of all layers
# together costs a few seconds): 6, 3.5 and 2 forward tiles per workgroup at 224, 112 and 56 on 256 CUs (>= 2 asserted below).
UNET_224_LAYERS = [
    (64, 64, 224, 16, 2, "pool_bits"),      # dconv_down1.2
    (64, 64, 224, 16, 2, "head"),           # dconv_up1.2 + conv_last
    (64, 128, 112, 16, 0, "bits"),          # dconv_down2.0
    (128, 128, 112, 16, 2, "pool_bits"),    # dconv_down2.2
    (128, 128, 112, 16, 2, "plain"),        # dconv_up2.2
    (128, 256, 56, 16, 0, "bits"),          # dconv_down3.0
    (256, 256, 56, 16, 2, "pool_bits"),     # dconv_down3.2
    (256, 256, 56, 16, 2, "plain"),         # dconv_up3.2
    (256, 512, 28, 16, 0, "bits"),          # dconv_down4.0: exactly one tile per CU, runs as it is
    (512, 512, 28, 16, 2, "plain"),         # dconv_down4.2
    (768, 256, 56, 16, 0, "bits"),          # dconv_up3.0
    (384, 128, 112, 16, 0, "bits"),         # dconv_up2.0
    (192, 64, 224, 16, 0, "bits"),          # dconv_up1.0: the input is the concat buffer, written as its two channel slices
]


@pytest.mark.parametrize("layer", UNET_224_LAYERS, ids=lambda l: f"{l[0]}-{l[1]}@{l[2]}-{l[5]}")
def test_unet_layers_at_224_are_exact(layer):
    """Every distinct 3x3 layer of Conditional_UNet at 224 x 224 through the kernel calls the fused graph makes (wu/unet_graph.py): forward
    + ReLU in its graph form (gate bits for a block's first conv; pool + gate / arg-max bits, the fused head, or plain for its second),
    the data gradient (gated by the bits of the block's mid activation for a second conv, ungated for a first conv -- there the gate belongs
    to the max-pool backward -- and additionally gated by a tensor), and the weight gradient.  No option is touched."""
    from wu import kernels as K
    cin, cout, s, n, pos, form = layer
    dev = _dev()
    shape = (n, cin, cout, s, s)
    cus = _cu_count()
    if s >= 56:
        assert _ntiles(shape) >= 2 * cus, f"{_ntiles(shape)} forward tiles on {cus} CUs"
    _exact(9 * max(cin, cout) * 2 + 3)
    x = _ints((n, cin, s, s), -2, 2, 400)
    wt = _ints((cout, cin, 3, 3), -1, 1, 401)
    bias = _ints((cout,), -3, 3, 402)
    y_relu = F.relu(F.conv2d(x, wt, bias, padding=1)).bfloat16().to(dev)
    if cin == 192:
        xd = torch.full((n, s, s, cin), float("nan"), dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2)
        xd[:, :128].copy_(x[:, :128].to(dev))
        xd[:, 128:].copy_(x[:, 128:].to(dev))
    else:
        xd = _bf16_dev(x)
    bd = bias.to(dev)
    wf, wd = K.pack_conv3x3(wt.to(dev), K._lib.BF16)
    tag = f"{cin} -> {cout} @ {s} x {s}, B = {n}"

    # ---- forward ----
    assert K.gate_bits_supported(xd, _sliced(n, cout, s, s)[1])
    if form == "pool_bits":          # an encoder block's second conv writes its slice of the concat buffer (cunet.py:62)
        buf, y = _sliced(n, cout, s, s, lead=2 * cout, trail=0)
        pbuf, pool = _sliced(n, cout, s // 2, s // 2, lead=0, trail=0)
        gbuf, gb = _bits_buffer(n, cout, s, s)
        sbuf, sb = _bits_buffer(n, cout, s, s)
        K.conv3x3_relu_pool_bits(xd, wf, bd, y, pool, gb, sb)
        _check_slice(buf, cout, y_relu, f"{tag} forward + pool + bits", lead=2 * cout)
        pooled, sel = _pool_reference(y_relu)
        _check_slice(pbuf, cout, pooled, f"{tag} pooled", lead=0)
        assert torch.equal(_decode_bits(gb, n, cout, s, s), y_relu > 0), f"{tag}: gate bits"
        assert torch.equal(_decode_bits(sb, n, cout, s, s), sel), f"{tag}: arg-max bits"
        _check_guards(gbuf, tag)
        _check_guards(sbuf, tag)
        del sel, pooled
    elif form == "bits":
        buf, y = _sliced(n, cout, s, s, lead=0, trail=0)
        gbuf, gb = _bits_buffer(n, cout, s, s)
        K.conv3x3_bits(xd, wf, bd, y, K.ACT_RELU, gate_bits_out=gb)
        _check_slice(buf, cout, y_relu, f"{tag} forward + gate bits", lead=0)
        assert torch.equal(_decode_bits(gb, n, cout, s, s), y_relu > 0), f"{tag}: gate bits"
        _check_guards(gbuf, tag)
    elif form == "head":
        assert K.conv3x3_head_supported(xd)
        g = torch.Generator().manual_seed(403)
        hw_ = ((torch.rand((3, 64), generator=g) * 2 - 1) * 0.006).to(dev)
        hb = ((torch.rand((3,), generator=g) * 2 - 1) * 0.3).to(dev)
        buf, y = _sliced(n, cout, s, s, lead=0, trail=0)
        out = torch.full((n, 3, s, s), float("nan"), device=dev)
        K.conv3x3_relu_head(xd, wf, bd, y, hw_, hb, out)
        _check_slice(buf, cout, y_relu, f"{tag} forward + head", lead=0)
        z = torch.einsum("kc,nchw->nkhw", hw_.double().cpu(), y_relu.double().cpu()) + hb.double().cpu().view(1, 3, 1, 1)
        assert float((torch.tanh(z).abs() < 0.9).double().mean()) > 0.5, "head reference saturated"
        err = (out.double().cpu() - torch.tanh(z)).abs().max().item()
        assert err < 2e-6, f"{tag}: head vs float64 {err}"
    else:
        buf, y = _sliced(n, cout, s, s, lead=0, trail=0)
        K.conv3x3(xd, wf, bd, y, 1, K.ACT_RELU)
        _check_slice(buf, cout, y_relu, f"{tag} forward", lead=0)
    del buf, y

    # ---- data gradient: gy (Cout channels) -> dx (Cin channels) on the rotated pack ----
    gy = _ints((n, cout, s, s), -1, 1, 404)
    gyd = _bf16_dev(gy)
    dx = torch.nn.grad.conv2d_input((n, cin, s, s), wt, gy, padding=1)
    gate = _ints((n, cin, s, s), -2, 2, 405).to(dev)
    dx_dev = dx.to(dev)
    dx_gated = (dx_dev * (gate > 0)).bfloat16()
    assert K.gate_bits_supported(gyd, _sliced(n, cin, s, s, 0, 0)[1])
    if pos == 0:
        buf, d = _sliced(n, cin, s, s, lead=0, trail=0)
        K.conv3x3(gyd, wd, None, d)
        _check_slice(buf, cin, dx_dev.bfloat16(), f"{tag} data gradient", lead=0)
    else:
        buf, d = _sliced(n, cin, s, s, lead=0, trail=0)
        K.conv3x3_bits(gyd, wd, None, d, K.ACT_NONE, egate_bits=_encode_bits(gate > 0))
        _check_slice(buf, cin, dx_gated, f"{tag} data gradient gated by bits", lead=0)
    buf, d = _sliced(n, cin, s, s, lead=0, trail=0)
    K.conv3x3(gyd, wd, None, d, 1, K.ACT_NONE, egate=gate.bfloat16().contiguous(memory_format=torch.channels_last), egate_act=K.ACT_RELU)
    _check_slice(buf, cin, dx_gated, f"{tag} data gradient gated by a tensor", lead=0)
    del buf, d, dx, dx_dev, dx_gated, gate

    # ---- weight gradient (the graph passes the pre-gated gradient) ----
    _exact(n * s * s * 2 + 8)
    dw_ref = torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), gy, padding=1).to(dev)
    db_ref = gy.sum(dim=(0, 2, 3)).to(dev)
    if _wgrad_v2_eligible(s, s, cin, cout):
        assert _wgrad_v2_plan(n, s, s, cin, cout, cus)[2] >= 3       # W = 224: several tiles per split on the whole chip
    _run_wgrad(xd, gyd, None, dw_ref, db_ref, f"{tag} weight gradient")


def test_unet_at_224_is_deterministic_and_walk_independent():
    """Conditional_UNet at the reference's default shape (224 x 224, B = 16, bf16, train mode, fixed dropout seed): the forward and all 36
    gradients are bit-identical between two runs, and between the persistent walk and one tile per workgroup (WU_OPT_CONV_PERSISTENT = 0;
    the weight-gradient split counts do not depend on that option)."""
    import cunet
    from oracle import cunet_ref as O
    dev = _dev()
    nc = 5
    net = cunet.Conditional_UNet(nc, precision="bf16")
    net.load_state_dict(O.make_cunet_params(nc, 2), strict=True)
    net = net.to(dev).train()
    net.dropout_seed = 5
    g = torch.Generator().manual_seed(12)
    x = (torch.rand((16, 3, 224, 224), generator=g) * 2 - 1).to(dev)
    c = torch.eye(nc)[torch.arange(16) % nc].to(dev)

    def run():
        for p in net.parameters():
            p.grad = None
        out = net(x, c)
        torch.mean(torch.abs(out - x)).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    o1, g1 = run()
    o2, g2 = run()
    with _options({OPT_PERSISTENT: 0}):
        o3, g3 = run()
    assert len(g1) == 36
    assert not bool(torch.isnan(o1).any()) and float(o1.abs().max()) > 0
    assert torch.equal(o1, o2), "forward not reproducible"
    assert torch.equal(o1, o3), "forward differs between the persistent walk and one tile per workgroup"
    for k in g1:
        assert torch.equal(g1[k], g2[k]), f"gradient of {k} is not reproducible"
        assert torch.equal(g1[k], g3[k]), f"gradient of {k} differs between the persistent walk and one tile per workgroup"
