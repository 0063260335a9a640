"""Case tables, plan mirror, integer operands and the CPU oracle of tests/test_gpu_wgrad_exact.py (no GPU import; checked by
tests/test_wgrad_ref_cpu.py): the generic 3 x 3 weight gradient of csrc/conv3x3_wgrad.hip -- conv3x3_wgrad_kernel<bf16_t,2,128>,
<float,1,128>, <float,2,64>, <bf16_t,1,256> at tile widths below 32 -- and its reducer wgrad_reduce_kernel.

`wgrad_plan` / `reduce_plan` restate the host code (wgrad_plan, launch_wgrad_reduce) and the index arithmetic of wgrad_reduce_kernel in
plain Python.  The split count is ceil(512 / channel blocks) capped by the tile count: it depends neither on the CU count nor on option
10.  Every case names the plan features it is there for (`expect`), and `check_features` asserts them from the mirror, so a change of the
plan cannot quietly empty a case.

Operands are small integers (x in [-2, 2], dy in [-1, 1], y in [-2, 2] with exact zeros): products are exact, and an fp32 sum of
integers is exact in ANY order below 2^24, so torch's CPU fp32 conv2d_weight is the one right answer whatever the tile, split, MFMA shape
or reducer tree.  A LeakyReLU gate in bf16 stages round_bf16(0.2f dy): +-205/1024 for dy = +-1, so every product is a multiple of 2^-10
and the sums stay exact while 2 N Ho Wo 2^10 < 2^24.  In fp32 0.2f dy is no short dyadic number: no exact oracle, see `error_bound`."""
import collections
import functools

import torch
import torch.nn.functional as F

from _pointwise_ref import LEAKY, NONE, RELU, SLOPE, TWO24, act_gate, ints      # noqa: F401  (re-exported)

RX, RDY, RY = 2, 1, 2                            # |x|, |dy|, |y| at most
ACCUM = 8                                        # the integer-loaded gradients of the accumulate = 1 run: |dw0|, |db0| <= 5 < 8
LEAKY_BF16_UNIT = 2.0 ** -10                     # every value of round_bf16(0.2f * dy), dy = +-1, is a multiple of it (checked on the CPU)
INSTANCE = {("bf16", 1): "conv3x3_wgrad_kernel<bf16_t,1,256>", ("bf16", 2): "conv3x3_wgrad_kernel<bf16_t,2,128>",
            ("fp32", 1): "conv3x3_wgrad_kernel<float,1,128>", ("fp32", 2): "conv3x3_wgrad_kernel<float,2,64>"}
PIXELS = {("bf16", 1): 256, ("bf16", 2): 128, ("fp32", 1): 128, ("fp32", 2): 64}      # P: output pixels per tile
STAGE_REGS = {"bf16": 19, "fp32": 21}            # NX: 16-byte X items per thread of the stride-2 prefetch


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan mirror
# ---------------------------------------------------------------------------------------------------------------------------------
WPlan = collections.namedtuple("WPlan", "P TW TH ho wo tiles_x tiles_y ntiles splits tps_min tps_max halo_w halo_h lds ws stage_items stage_slots")
RPlan = collections.namedtuple("RPlan", "wpr c4n TX G trips group_counts")


def wgrad_plan(n, cin, cout, h, w, stride, dtype):
    """wgrad_plan of csrc/conv3x3_wgrad.hip, with the tiles each split walks (tile = split, split + splits, ...) and the staging items of
    the stride-2 prefetch (halo pixels x 16-byte slots of the 256 threads x NX registers the host checks)."""
    bf = dtype == "bf16"
    p = PIXELS[(dtype, stride)]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    twl = 5
    while twl > 2 and (1 << (twl - 1)) >= wo:
        twl -= 1
    tw, th = 1 << twl, p >> twl
    tiles_x, tiles_y = cdiv(wo, tw), cdiv(ho, th)
    ntiles = n * tiles_x * tiles_y
    blocks = (cout // 64) * (cin // 64)
    splits = max(1, min(cdiv(512, blocks), ntiles))
    halo_w, halo_h = (tw - 1) * stride + 3, (th - 1) * stride + 3
    rb = 128 if bf else 256
    lds = (p + halo_w * halo_h) * rb
    ws = (splits * 9 * cout * cin + splits * cout) * 4
    per_split = [len(range(s, ntiles, splits)) for s in range(splits)]
    return WPlan(p, tw, th, ho, wo, tiles_x, tiles_y, ntiles, splits, min(per_split), max(per_split), halo_w, halo_h, lds, ws,
                 halo_w * halo_h * (rb // 16), STAGE_REGS[dtype] * 256)


def launchable(plan, stride):
    """The two refusals of wu_conv3x3_wgrad that depend on the plan: LDS, and the stride-2 staging registers."""
    return plan.lds <= 160 * 1024 and (stride == 1 or plan.stage_items <= plan.stage_slots)


def reduce_plan(splits, cin):
    """launch_wgrad_reduce + wgrad_reduce_kernel: waves per (co, tap) row, float4 columns per wave, lanes across them, split groups, trips
    of the c4b loop, and how many splits each group adds (group g takes g, g + G, ...: an odd count ends in the `if (k < splits)` tail,
    a count of zero is a group with nothing to read)."""
    c4 = cin >> 2
    wpr = 1
    while wpr < 8 and splits * c4 > 64 * 16 * wpr and c4 % (2 * wpr) == 0:
        wpr <<= 1
    c4n = c4 // wpr
    tx = 64
    while tx > c4n:
        tx >>= 1
    g = 64 // tx
    return RPlan(wpr, c4n, tx, g, cdiv(c4n, tx), tuple(len(range(k, splits, g)) for k in range(g)))


def v2_eligible(h, w, cin, cout, stride, dtype, gated):
    """wgrad_v2_eligible (csrc/conv3x3_wgrad_v2.hip): the shapes the LDS-DMA kernel takes instead of the generic one."""
    return dtype == "bf16" and stride == 1 and not gated and w % 32 == 0 and cin % 64 == 0 and cout % 64 == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
WCase = collections.namedtuple("WCase", "name n cin cout h w stride dtype seed expect")
ALL = tuple((s, d) for s in (1, 2) for d in ("bf16", "fp32"))


def _expect(shape, stride, dtype):
    """Plan features a case is there for: field of WPlan / RPlan -> value (asserted by check_features)."""
    key = (stride, dtype)
    e = {}
    if shape in ((1, 64, 64, 1, 1), (1, 64, 64, 2, 2)):
        e.update(ntiles=1, splits=1, TW=4, G=4, wpr=1)             # splits = 1 < G = 4: three split groups with nothing to read
        if stride == 2:
            e.update(ho=1, wo=1)                                   # a single output pixel
    elif shape == (1, 128, 256, 5, 3):
        e.update(TW=4, TX=32, G=2)
    elif shape == (2, 64, 64, 7, 7):
        e.update(TW=8 if stride == 1 else 4)
        if key == (2, "bf16"):
            e.update(halo_w=9, halo_h=65, stage_items=585 * 8, stage_slots=608 * 8)
    elif shape == (3, 64, 128, 14, 14):
        e.update(TW=16 if stride == 1 else 8)
        if key == (1, "fp32"):
            e.update(TH=8, tiles_y=2)                              # 14 rows: the second tile row holds 6 of 8
    elif shape == (2, 128, 64, 13, 27):
        e.update(TW=32 if stride == 1 else 16)
        if stride == 2:
            e.update(wo=14, ho=7)
    elif shape == (2, 192, 64, 21, 35):
        e.update(TW=32)
        if stride == 1:
            e.update(tiles_x=2)                                    # the right tile column holds 3 of 32
        if key == (1, "fp32"):
            e.update(wpr=2, c4n=24, TX=16, trips=2)
        else:
            e.update(wpr=1, c4n=48, TX=32, trips=2)                # the second trip has lanes with valid = false
    elif shape == (3, 512, 512, 9, 11):
        e.update(wpr=1, c4n=128, TX=64, G=1, trips=2)
    elif shape == (9, 256, 256, 45, 79):
        e.update(wo=40, ho=23, TW=32, tiles_x=2, splits=32, wpr=2)
        e.update(dict(ntiles=108, tps_min=3, tps_max=4) if dtype == "bf16" else dict(ntiles=216, tps_min=6, tps_max=7))
    elif shape == (3, 256, 256, 45, 79):
        e.update(TW=32, tiles_x=3, ntiles=108, splits=32, tps_min=3, tps_max=4)
    elif shape == (40, 64, 64, 45, 79):
        e.update(ntiles=480, splits=480, wpr=8, c4n=2, TX=2, G=32, tps_max=1)
    elif shape == (130, 64, 64, 7, 7):
        e.update(TW=8, ntiles=130, splits=130, wpr=4, c4n=4, TX=4, G=16, group_counts=(9, 9) + (8,) * 14)
    return e


def _cases():
    table = [((1, 64, 64, 1, 1), ALL), ((1, 64, 64, 2, 2), ALL), ((1, 128, 256, 5, 3), ALL), ((2, 64, 64, 7, 7), ALL), ((3, 64, 128, 14, 14), ALL),
             ((2, 128, 64, 13, 27), ALL), ((2, 192, 64, 21, 35), ALL), ((3, 512, 512, 9, 11), ALL),
             ((9, 256, 256, 45, 79), ((2, "bf16"), (2, "fp32"))),          # the walk: several tiles per split, uneven
             ((3, 256, 256, 45, 79), ((1, "fp32"),)),                      # the same walk for <float,1,128>
             ((40, 64, 64, 45, 79), ((2, "bf16"),)),                       # the reducer at its widest
             ((130, 64, 64, 7, 7), ((1, "bf16"),))]                        # wpr = 4 (Cin = 64 takes it at 129..256 splits); odd and even group counts in one row
    out = []
    for i, (shape, combos) in enumerate(table):
        for stride, dtype in combos:
            name = "x".join(str(v) for v in shape) + f"-s{stride}-{dtype}"
            out.append(WCase(name, *shape, stride, dtype, 7000 + 10 * i, tuple(sorted(_expect(shape, stride, dtype).items()))))
    return out


CASES = _cases()
SMALL_SHAPES = 8                                 # the first eight shapes run all four instances: the gated tests use them


def plans(c):
    p = wgrad_plan(c.n, c.cin, c.cout, c.h, c.w, c.stride, c.dtype)
    return p, reduce_plan(p.splits, c.cin)


def check_features(c):
    """The plan features this case was written for, from the mirror; the shape is one the generic kernel takes and can launch."""
    p, r = plans(c)
    both = {**p._asdict(), **r._asdict()}
    for k, v in c.expect:
        assert both[k] == v, f"{c.name}: plan {k} = {both[k]}, the case was written for {v}"
    assert launchable(p, c.stride), f"{c.name}: {p}"
    assert not v2_eligible(c.h, c.w, c.cin, c.cout, c.stride, c.dtype, False), f"{c.name}: the LDS-DMA kernel would take it"
    assert c.cin % 64 == 0 and c.cout % 64 == 0
    return p, r


def gate_cases(act, dtype=None):
    """The cases of the in-kernel gate: the eight small shapes, every instance (LeakyReLU: bf16 only, where the oracle is exact)."""
    small = [c for c in CASES if c.seed < 7000 + 10 * SMALL_SHAPES]
    if act == LEAKY and dtype is None:
        dtype = "bf16"
    return [c for c in small if dtype is None or c.dtype == dtype]


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, bounds, oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def bound(c, act=NONE):
    """Worst-case |sum| in units of the smallest product: 2 per pixel (|x| <= 2, |dy'| <= 1) + the accumulate load; a bf16 LeakyReLU
    gate makes the unit 2^-10."""
    p, _ = plans(c)
    pix = c.n * p.ho * p.wo
    if act == LEAKY:
        assert c.dtype == "bf16", "no exact oracle for a LeakyReLU gate in fp32"
        return (RX * RDY * pix + ACCUM) * 2 ** 10
    return RX * RDY * pix + ACCUM


@functools.lru_cache(maxsize=4)
def operands(c):
    p, _ = plans(c)
    x = ints((c.n, c.cin, c.h, c.w), -RX, RX, c.seed)
    dy = ints((c.n, c.cout, p.ho, p.wo), -RDY, RDY, c.seed + 1)
    y = ints((c.n, c.cout, p.ho, p.wo), -RY, RY, c.seed + 2)
    return x, dy, y


def gated(dy, y, act, dtype):
    """dy' as the kernel stages it: one fp32 multiply (LeakyReLU), one rounding to the operand type."""
    g = act_gate(dy, y, act)
    return g.bfloat16().float() if dtype == "bf16" else g


def dw_db(x, g, c, acc=torch.float32):
    dw = torch.nn.grad.conv2d_weight(x.to(acc), (c.cout, c.cin, 3, 3), g.to(acc), stride=c.stride, padding=1)
    return dw, g.to(acc).sum((0, 2, 3))


def tap_terms(c):
    """(3, 3) float64: the summands each tap of one (co, ci) element has -- the output pixels whose tap lies inside the image (a weight
    gradient of ones).  A one-pixel image has a single tap with any."""
    p, _ = plans(c)
    one = c._replace(cin=1, cout=1)
    return dw_db(torch.ones((c.n, 1, c.h, c.w)), torch.ones((c.n, 1, p.ho, p.wo)), one, torch.float64)[0].view(3, 3)


@functools.lru_cache(maxsize=None)
def reference(c, act=NONE):
    """(dw (Cout, Cin, 3, 3), db (Cout,)) in fp32 on the CPU; cached per (case, gate)."""
    x, dy, y = operands(c)
    return dw_db(x, gated(dy, y, act, c.dtype) if act != NONE else dy, c)


def error_bound(c, act):
    """(dw64, db64, bound_dw, bound_db) for a gate without an exact oracle (LeakyReLU in fp32): the float64 result on the fp32-gated
    gradient, and per element n_terms 2^-24 sum |x dy'| -- the forward error bound of an fp32 sum of n_terms exact products in any
    order (n_terms from a weight gradient of ones: the pixels a tap really has)."""
    x, dy, y = operands(c)
    g = gated(dy, y, act, c.dtype)
    dw64, db64 = dw_db(x, g, c, torch.float64)
    sabs, babs = dw_db(x.abs(), g.abs(), c, torch.float64)
    return dw64, db64, tap_terms(c).view(1, 1, 3, 3) * 2.0 ** -24 * sabs, g[:, 0].numel() * 2.0 ** -24 * babs


def memory_order_border_dw(c, x, g, acc=torch.float64):
    """(dw with zero padding written out by hand, dw with the WRONG border rule a strided address walk gives): the column right of the
    image is the first column of the next row of memory, the row below the image is the first row of the next image."""
    n, _, h, w = x.shape
    pad = F.pad(x.to(acc), (1, 1, 1, 1))
    wrong = pad.clone()
    wrong[:, :, 1:h, w + 1] = x[:, :, 1:, 0].to(acc)          # (row i, column W) := (row i + 1, column 0)
    wrong[:-1, :, h + 1, 1:w + 1] = x[1:, :, 0, :].to(acc)    # (image n, row H) := (image n + 1, row 0)
    wrong[:-1, :, h, w + 1] = x[1:, :, 0, 0].to(acc)          # (image n, row H - 1, column W) := (image n + 1, row 0, column 0)
    f = lambda t: torch.nn.grad.conv2d_weight(t, (c.cout, c.cin, 3, 3), g.to(acc), stride=c.stride, padding=0)      # noqa: E731
    return f(pad), f(wrong)


# ---------------------------------------------------------------------------------------------------------------------------------
# wu_act_gate alone, and the y-gated scatter of wu_conv3x3_s2_dgrad
# ---------------------------------------------------------------------------------------------------------------------------------
ACT_GATE_GRID_ITEMS = 256 * 8192                 # threads of act_gate_kernel's largest grid: more items make the grid-stride loop turn
# (N, C, H, W) per dtype: a few pixels; one 16-byte slot per pixel; more items than the largest grid
ACT_GATE_SHAPES = {"bf16": ((1, 64, 1, 3), (2, 8, 5, 7), (4, 64, 256, 257)), "fp32": ((1, 64, 1, 3), (2, 4, 5, 7), (2, 64, 256, 257))}
ACT_GATE_PADS = ((0, 0, 0), (8, 16, 24), (24, 8, 0))      # extra channels of the buffers of g, y, out: three different pixel strides


def act_gate_operands(shape, seed, integers):
    """g and y: integers (exact in bf16), or reals on the bf16 grid times 1/7-ish factors (0.2f g then needs its one rounding)."""
    if integers:
        return ints(shape, -9, 9, seed), ints(shape, -RY, RY, seed + 1)
    gen = torch.Generator().manual_seed(seed)
    g = ((torch.rand(shape, generator=gen) * 2 - 1) * 3).bfloat16().float()
    y = ((torch.rand(shape, generator=gen) * 2 - 1)).bfloat16().float()
    y[..., ::5] = 0
    return g, y


def act_gate_reference(g, y, act, dtype):
    """torch.where(y > 0, g, g.float() * SLOPE).to(dtype): one fp32 multiply, one rounding."""
    return act_gate(g, y, act).to(dtype)


S2_UP_GRID_ITEMS = 256 * 4096                    # threads of upsample_zero_gate_kernel's largest grid
S2_RDY, S2_RW = 2, 2
S2Gate = collections.namedtuple("S2Gate", "name n cin cout h w seed")
# two odd-sized shapes of _pointwise_ref.S2_CASES, and one whose N H W Cout / E exceeds the largest grid in both precisions
S2_GATE_CASES = [S2Gate("3x64x128x5x7", 3, 64, 128, 5, 7, 7501), S2Gate("1x128x64x11x13", 1, 128, 64, 11, 13, 7502),
                 S2Gate("1x64x64x363x365", 1, 64, 64, 363, 365, 7503)]


def s2_gate_bound(c, act):
    """Worst-case |dx|: nine taps x Cout products of |w| <= 2 and |dy'| <= 2, in units of 2^-10 under a bf16 LeakyReLU gate
    (round_bf16(0.2f dy) for |dy| in {1, 2} is a multiple of 2^-10: asserted on the CPU)."""
    return 9 * c.cout * S2_RDY * S2_RW * (2 ** 10 if act == LEAKY else 1)


def s2_gate_operands(c):
    ho, wo = (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
    w = ints((c.cout, c.cin, 3, 3), -S2_RW, S2_RW, c.seed)
    dy = ints((c.n, c.cout, ho, wo), -S2_RDY, S2_RDY, c.seed + 1)
    y = ints((c.n, c.cout, ho, wo), -RY, RY, c.seed + 2)
    return dict(w=w, dy=dy, y=y)
