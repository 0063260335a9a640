"""Case tables, integer operands, the CPU oracle and the launch plans of tests/test_gpu_conv_s1_exact.py (no GPU import; checked by
tests/test_conv_s1_ref_cpu.py): the register-staged template conv3x3_mfma_kernel<T, 1, MASKED> of csrc/conv3x3_mfma.hip at stride 1 and the
small-image kernel conv3x3_small_kernel<NHK, D> of csrc/conv3x3_small.hip.

The oracle is the one of tests/_pointwise_ref.py: operands are small integers, bf16 x bf16 products are exact in fp32, mfma_f32_32x32x2f32 is
exact on integers, and an fp32 sum of integers is exact in ANY order while it stays below 2^24 -- so F.conv2d in fp32 on the CPU is the one
right answer for the sum whatever the tile, chunk order, ring depth or K split.  Every case states its worst-case bound (`s1_bound`).

The epilogue order is the kernels': bias, activation, ONE rounding to the storage type; an output gate is then applied to the STORED value
and the result is rounded AGAIN (gate16<T> of csrc/wu_common.h on the packed tile: ConvArgs::late_gate == 0, the two roundings of the
stand-alone gate pass that wu/disc_graph.py relies on).  A ReLU gate keeps or drops a stored value, so its second rounding changes nothing;
a leaky gate multiplies the stored bf16 value by 0.2f and rounds the product.

The input mask (MASKED, mask_act) stages gate16(x, mask).  With a ReLU mask the operands stay integers.  With a leaky mask in bf16 they
become bf16(0.2f * k): for |k| <= 4 a multiple of 2^-10 (0.2 -> 205 * 2^-10, 0.4 -> 205 * 2^-9, 0.6 -> 154 * 2^-8, 0.8 -> 205 * 2^-8), so the sum
is still exact in fp32 while 2^10 * bound < 2^24 (`s1_bound` carries the factor).  A leaky mask in fp32 produces 24-bit operands whose sum
is not order-independent: that ONE combination stays with the tolerance test tests/test_gpu_kernels.py::test_conv3x3_gated_abi_paths (no network
passes a mask: it is an ABI path only)."""
import collections

import torch
import torch.nn.functional as F

from _pointwise_ref import LEAKY, NONE, PW_RW, PW_RX, RB, RELU, RG, SLOPE, TWO24, act_apply, act_gate, ints, unrepresentable  # noqa: F401

OPT_CONV_V2, OPT_CONV_SMALL, OPT_GRID = 0, 3, 10         # wu_set_option keys (csrc/wu_common.h)
DEFAULTS = {OPT_CONV_V2: 1, OPT_CONV_SMALL: 1, OPT_GRID: 0}      # csrc/wu_prof.hip
CHUNK = {"bf16": 32, "fp32": 16}                         # channels per 64-byte K chunk
LEAKY_MASK_RX = 4                                        # |x| at most, where a leaky mask scales it (module docstring)


def _cdiv(a, b):
    return -(-a // b)


def _round(v32, dtype):
    """One rounding to the storage type and back to fp32."""
    assert v32.dtype == torch.float32
    return v32.bfloat16().float() if dtype == "bf16" else v32


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch plans, restated
# ---------------------------------------------------------------------------------------------------------------------------------
TemplatePlan = collections.namedtuple("TemplatePlan", "tw_log2 TH tiles_y tiles_x halo_pix nchunks")
SmallPlan = collections.namedtuple("SmallPlan", "tw_log2 ipt tiles_y tiles_x halo_pix nhk depth nchunks groups")
SMALL_MAX_NHK = 5


def template_plan(H, W, Cin, dtype):
    """conv3x3_fwd_dispatch at stride 1: 256 output pixels per workgroup as TH x TW, TW = 32 / 16 / 8 / 4 for W > 16 / 9..16 / 5..8 / <= 4."""
    twl = 5
    while twl > 2 and (1 << (twl - 1)) >= W:
        twl -= 1
    TW, TH = 1 << twl, 256 >> twl
    return TemplatePlan(twl, TH, _cdiv(H, TH), _cdiv(W, TW), (TW + 2) * (TH + 2), Cin // CHUNK[dtype])


def small_plan(N, H, W, Cin, Cout):
    """conv_small_launch: 128 output pixels per workgroup; images shorter than the tile are stacked, each with its own halo rows, while the
    stacked halo image fits 320 pixels.  None where the shape is outside the kernel's ABI; nhk > SMALL_MAX_NHK means it declines too."""
    if W > 16 or Cin % 32 != 0 or Cout % 64 != 0:
        return None
    twl = 4 if W > 8 else (3 if W > 4 else 2)
    TW, TH = 1 << twl, 128 >> twl
    ipt = TH // H if H < TH else 1
    ipt = max(ipt, 1)
    while ipt > 1 and ipt * (H + 2) * (TW + 2) > 320:
        ipt -= 1
    tiles_y = 1 if ipt > 1 else _cdiv(H, TH)
    halo_h = ipt * (H + 2) if ipt > 1 else TH + 2
    halo_pix = (TW + 2) * halo_h
    nhk = _cdiv(_cdiv(halo_pix, 16), 4)
    return SmallPlan(twl, ipt, tiles_y, _cdiv(W, TW), halo_pix, nhk, 3 if nhk <= 4 else 2, Cin // 32, _cdiv(N, ipt) if ipt > 1 else N)


def small_instance(plan):
    """The template instance <NHK, D> conv_small_launch picks."""
    return (3, 3) if plan.nhk <= 3 else ((4, 3) if plan.nhk == 4 else (5, 2))


def small_rows_valid(plan, H):
    """Tile rows that hold output pixels (the kernel's rows_valid); the others meet the `ry = min(ry, rows_valid - 1)` clamp."""
    return plan.ipt * H if plan.ipt > 1 else 128 >> plan.tw_log2


def small_preferred(N, H, W, Cin, Cout, cus, opt3=1):
    """wu_conv3x3_small_supported: the shape is the small kernel's AND the dispatch rule prefers it to the template -- where the template's
    256-pixel tiles lie inside the image (W > 8: a 16-wide tile is 16 rows) and fill three quarters of the chip, the template is chosen."""
    p = small_plan(N, H, W, Cin, Cout)
    if not opt3 or p is None or p.nhk > SMALL_MAX_NHK:
        return False
    if W > 8 and H >= 16 and opt3 != 2 and N * _cdiv(H, 16) * (Cout // 64) * 4 >= 3 * cus:
        return False
    return True


def v2_eligible(H, W, Cin, Cout, dtype, masked):
    """conv_v2_eligible at stride 1, for tensors far below its 2^31-byte limits."""
    return dtype == "bf16" and not masked and 16 < W <= 4096 and Cin % 32 == 0 and Cin >= 64 and Cout % 64 == 0


def dispatch(dtype, N, H, W, Cin, Cout, has_bias, act, gated, masked, opts=None, cus=256):
    """Which kernel conv3x3_fwd_dispatch launches at stride 1: "v2" (conv3x3_mfma_v2_kernel), "small" or "template"."""
    o = {**DEFAULTS, **(opts or {})}
    if o[OPT_CONV_V2] and v2_eligible(H, W, Cin, Cout, dtype, masked) and (not gated or (act == NONE and not has_bias)):
        return "v2"
    if dtype == "bf16" and not masked and small_preferred(N, H, W, Cin, Cout, cus, o[OPT_CONV_SMALL]):
        return "small"
    return "template"


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogues: name -> (bias, activation, output gate, input mask, data-gradient form on the rotated pack)
# ---------------------------------------------------------------------------------------------------------------------------------
EPILOGUES = {
    "none": (False, NONE, NONE, NONE, False),
    "bias": (True, NONE, NONE, NONE, False),
    "bias_relu": (True, RELU, NONE, NONE, False),
    "bias_leaky": (True, LEAKY, NONE, NONE, False),
    "gate_relu": (False, NONE, RELU, NONE, True),
    "gate_leaky": (False, NONE, LEAKY, NONE, True),
    "bias_relu_gate": (True, RELU, RELU, NONE, False),
    "mask_relu": (False, NONE, NONE, RELU, False),
    "mask_leaky": (False, NONE, NONE, LEAKY, False),       # bf16 only (module docstring)
}
TEMPLATE_EPILOGUES = {"fp32": ["bias", "bias_relu", "bias_leaky", "gate_relu", "gate_leaky", "bias_relu_gate", "mask_relu"],
                      "bf16": ["bias", "bias_relu", "bias_leaky", "gate_relu", "gate_leaky", "bias_relu_gate", "mask_relu", "mask_leaky"]}
SMALL_EPILOGUES = ["bias_relu", "bias_leaky", "none", "gate_relu", "gate_leaky"]

# What sends a bf16 call to the template, and the options that route needs.  fp32 and a masked input always run there.
ROUTES = {
    "fp32": {},
    "mask": {},
    "cin32": {},                         # Cin == 32 with W > 16: below the LDS-DMA conv's Cin >= 64
    "gate_epilogue": {},                 # an output gate with a bias / activation on a shape the LDS-DMA conv would otherwise take
    "opt0": {OPT_CONV_V2: 0},            # a plain W > 16 shape with the LDS-DMA conv switched off
    "opt3": {OPT_CONV_SMALL: 0},         # W <= 16 with the small-image kernel switched off
}

S1Case = collections.namedtuple("S1Case", "name dtype n cin cout h w epi route seed")


def _case(dtype, n, cin, cout, h, w, epi, route, seed):
    return S1Case(f"{dtype}-{n}x{cin}x{cout}x{h}x{w}-{epi}-{route}", dtype, n, cin, cout, h, w, epi, route, seed)


# (N, Cin, Cout, H, W), epilogue[, route].  Tile = TH x TW: 8 x 32, 16 x 16, 32 x 8, 64 x 4 -- only the 32-wide tile can have a second tile column
# (W <= 16 is one tile of the width that fits it), every width has a case with two tile rows, a ragged last row and ragged columns.
_TEMPLATE_FP32 = [
    ((3, 48, 192, 9, 35), "bias_relu"),          # 32-wide: 2 x 2 tiles ragged both ways, three chunks, three cout tiles, N = 3
    ((1, 16, 64, 70, 3), "bias"),                # 4-wide: two tile rows (64 + 6), W = 3, ONE chunk (no store_chunk in the loop)
    ((2, 32, 64, 19, 12), "bias_leaky"),         # 16-wide: two tile rows (16 + 3), W = 12, two chunks (store_chunk once)
    ((1, 32, 64, 35, 7), "gate_relu"),           # 8-wide: two tile rows (32 + 3), W = 7
    ((1, 64, 64, 17, 33), "gate_leaky"),         # 32-wide: three tile rows, the second tile column one pixel wide, four chunks
    ((3, 32, 192, 5, 20), "bias_relu_gate"),     # 32-wide: one ragged tile, three cout tiles
    ((2, 48, 64, 33, 6), "mask_relu"),           # 8-wide, masked input, three chunks
    ((1, 16, 64, 8, 32), "bias_relu"),           # exactly one full tile
]
_TEMPLATE_BF16 = [
    ((3, 32, 64, 21, 40), "bias_relu", "cin32"),             # 32-wide: 3 x 2 tiles ragged both ways, ONE chunk, N = 3
    ((1, 64, 192, 9, 35), "bias_relu_gate", "gate_epilogue"),  # two chunks, three cout tiles
    ((2, 96, 64, 17, 33), "bias_leaky", "opt0"),             # three chunks, three tile rows
    ((1, 32, 64, 70, 3), "bias", "opt3"),                    # 4-wide, two tile rows
    ((2, 64, 64, 19, 12), "gate_relu", "opt3"),              # 16-wide, two tile rows
    ((3, 96, 192, 35, 7), "gate_leaky", "opt3"),             # 8-wide, two tile rows, three chunks, three cout tiles
    ((2, 64, 64, 9, 20), "mask_relu", "mask"),
    ((1, 32, 64, 12, 18), "mask_leaky", "mask"),             # Cin = 32: 2^10 x bound stays below 2^24
    ((1, 128, 64, 8, 32), "gate_leaky", "opt0"),             # exactly one full tile, four chunks
]


def _template_cases():
    out, seed = [], 6000
    for shape, epi in _TEMPLATE_FP32:
        seed += 1
        out.append(_case("fp32", *shape, epi, "fp32", seed))
    for shape, epi, route in _TEMPLATE_BF16:
        seed += 1
        out.append(_case("bf16", *shape, epi, route, seed))
    return out


TEMPLATE_CASES = _template_cases()

# The small-image kernel: (N, Cin, Cout, H, W), epilogue.  The notes are re-derived from small_plan by tests/test_conv_s1_ref_cpu.py.
_SMALL = [
    ((5, 256, 256, 16, 16), "bias_relu"),        # <3,3>: 16-wide, one image = two row tiles, eight chunks, four cout tiles
    ((5, 128, 64, 8, 8), "bias_leaky"),          # <4,3>: two 8x8 images per tile, three groups, the last half empty; four chunks
    ((7, 96, 64, 5, 3), "gate_relu"),            # <4,3>: 4-wide, six 5-row images per 32-row tile (two unused rows), the second group holds one; three chunks
    ((40, 64, 64, 2, 2), "gate_leaky"),          # <5,2>: thirteen 2x2 images per tile (the 320-pixel cap), four groups; two chunks
    ((1, 32, 64, 1, 1), "bias_relu"),            # <5,2>: seventeen single pixels per tile (cap), one present; ONE chunk
    ((3, 64, 64, 2, 16), "none"),                # <5,2>: four 2-row images fill the 8-row tile, N = 3
    ((2, 64, 64, 40, 4), "bias_leaky"),          # <4,3>: 4-wide, two row tiles per image (32 + 8); two chunks
    ((2, 128, 128, 24, 16), "gate_leaky"),       # <3,3>: three row tiles per image, two cout tiles
    ((3, 32, 64, 8, 8), "gate_relu"),            # <4,3>: ONE chunk at ring depth 3
    ((3, 64, 64, 7, 13), "bias_relu"),           # <3,3>: one row tile per image, ragged in H and W inside the tile
    ((9, 96, 64, 2, 7), "none"),                 # <5,2>: eight 2-row images per 8-wide tile, three chunks at ring depth 2, the second group holds one
]
SMALL_CASES = [_case("bf16", *shape, epi, "small", 7100 + i) for i, (shape, epi) in enumerate(_SMALL)]


# ---------------------------------------------------------------------------------------------------------------------------------
# operands and the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def s1_rx(c):
    return LEAKY_MASK_RX if EPILOGUES[c.epi][3] == LEAKY else PW_RX


def s1_bound(c):
    """Worst-case |sum + bias| in units of the operands' grid: 9 * Cin * max|x| * max|w| + max|bias|, where a planted bias cancels a sum and
    is at most the sum's own bound; x 2^10 where a leaky bf16 mask puts the staged operands on the 2^-10 grid."""
    has_b, _, _, mact, _ = EPILOGUES[c.epi]
    s = 9 * c.cin * s1_rx(c) * PW_RW
    b = s + (max(s, RB) if has_b else 0)
    return b * 1024 if mact == LEAKY else b


def s1_operands(c):
    """x (N, Cin, H, W); w OIHW of the conv this call computes -- for the data-gradient form the forward conv's weight (Cin, Cout, 3, 3),
    whose rotated pack the kernel reads; bias / gate (N, Cout, H, W) / mask (N, Cin, H, W) or None.  Every 8th bias cancels the sum of its
    channel's first site: exact zeros in front of the activation whatever the size."""
    has_b, _, gact, mact, dgrad = EPILOGUES[c.epi]
    assert not (dgrad and has_b)
    x = ints((c.n, c.cin, c.h, c.w), -s1_rx(c), s1_rx(c), c.seed)
    w = ints((c.cin, c.cout, 3, 3) if dgrad else (c.cout, c.cin, 3, 3), -PW_RW, PW_RW, c.seed + 10000)
    mask = ints((c.n, c.cin, c.h, c.w), -RG, RG, c.seed + 20000) if mact != NONE else None
    gate = ints((c.n, c.cout, c.h, c.w), -RG, RG, c.seed + 30000) if gact != NONE else None
    bias = None
    if has_b:
        bias = ints((c.cout,), -RB, RB, c.seed + 40000)
        bias[::8] = -F.conv2d(x, w, None, padding=1)[0, ::8, 0, 0]
    return dict(x=x, w=w, bias=bias, gate=gate, mask=mask)


def s1_staged(c, ops):
    """What the kernel multiplies: x, or gate16(x, mask) rounded to the storage type."""
    mact = EPILOGUES[c.epi][3]
    assert not (mact == LEAKY and c.dtype == "fp32"), "a leaky mask in fp32 has no exact oracle (module docstring)"
    return ops["x"] if mact == NONE else _round(act_gate(ops["x"], ops["mask"], mact), c.dtype)


def s1_reference(c, ops, acc=torch.float32):
    """(lin, pre, out) in fp32: the sum + bias; the value that meets the FIRST rounding; the value that meets the LAST one (the gated stored
    value where there is an output gate, else `pre` again).  The kernel's output is out rounded to the storage type."""
    has_b, act, gact, _, dgrad = EPILOGUES[c.epi]
    xs, w = s1_staged(c, ops).to(acc), ops["w"].to(acc)
    if dgrad:
        lin = torch.nn.grad.conv2d_input((c.n, c.cout, c.h, c.w), w, xs, padding=1)
    else:
        lin = F.conv2d(xs, w, ops["bias"].to(acc) if has_b else None, padding=1)
    lin = lin.float()
    pre = act_apply(lin, act)
    out = act_gate(_round(pre, c.dtype), ops["gate"], gact) if gact != NONE else pre
    return lin, pre, out


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatch rule's probes (predicate only: nothing is launched at these batch sizes)
# ---------------------------------------------------------------------------------------------------------------------------------
def rule_probes(cus):
    """[(N, H, W, Cin, Cout)]: a 16 x 16 image on each side of the threshold N * 4 >= 3 * CUs, and an 8-wide image the rule never sends away."""
    n_template = _cdiv(3 * cus, 4)
    return [(n_template, 16, 16, 64, 64), (n_template - 1, 16, 16, 64, 64), (4 * cus, 16, 8, 64, 64)]
