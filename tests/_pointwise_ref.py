"""Case tables, integer operands and the CPU oracle of tests/test_gpu_pointwise_exact.py (no GPU import; checked by
tests/test_pointwise_ref_cpu.py): the estimator's pointwise GEMM family and stem of csrc/resnet.hip.

Operands are small integers: bf16 holds integers up to 256 exactly, bf16 x bf16 products are exact in fp32, mfma_f32_32x32x2f32 is exact on
integers, and an fp32 sum of integers is exact in ANY order while it stays below 2^24.  So torch's CPU fp32 result is the one right answer
for the fp32 sum whatever the tile, K order, ring depth, wave count or split; every case states its worst-case bound (`*_bound`).
The epilogue order is the kernels': bias, + residual, activation, gate, then ONE rounding.  LeakyReLU (v > 0 ? v : 0.2f v) and the leaky
gate (y > 0 ? g : 0.2f g) are one fp32 multiply on an exact operand: written here with torch.where and a float32 0.2, the same single
operation.  The linear part (sum + bias + residual) can be computed in float64 (`acc`) to show that fp32 lost nothing."""
import collections

import torch
import torch.nn.functional as F

NONE, RELU, LEAKY = 0, 1, 2                      # wu/_lib.py ACT_*
TWO24 = 2 ** 24
RX, RW, RB, RR, RG = 8, 4, 16, 256, 2            # |x|, |w| (the chain; the other families widen them below), |bias|, |residual|, |gate| at most
PW_RX, PW_RW = 16, 8                             # the pointwise cases: without a residual, sums of 64 products of the narrower ranges rarely leave bf16
SLOPE = torch.tensor(0.2, dtype=torch.float32)


def ints(shape, lo, hi, seed):
    """Seeded integers in [lo, hi] as fp32 (exact in bf16 up to 256)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def act_apply(v, act):
    assert v.dtype == torch.float32
    if act == RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == LEAKY:
        return torch.where(v > 0, v, v * SLOPE)
    return v


def act_gate(g, y, act):
    assert g.dtype == torch.float32
    if act == RELU:
        return torch.where(y > 0, g, torch.zeros_like(g))
    if act == LEAKY:
        return torch.where(y > 0, g, g * SLOPE)
    return g


def unrepresentable(v32):
    """Fraction of fp32 values that bf16 cannot hold: where the rounding mode shows."""
    return float((v32.bfloat16().float() != v32).double().mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# conv1x1_mfma_kernel / conv1x1_pw3_kernel: the GEMM with its epilogue, the stride-2 gather and scatter
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> (bias, residual, activation, gate activation)
EPILOGUES = {
    "bias": (True, False, NONE, NONE),
    "bias_res_relu": (True, True, RELU, NONE),
    "gate": (False, False, NONE, RELU),
    "res_gate": (False, True, NONE, RELU),
    "leaky": (True, False, LEAKY, NONE),
    "leaky_gate": (False, False, NONE, LEAKY),
    "bare": (False, False, NONE, NONE),          # the scatter alone
}
EPI_ORDER = ["bias", "bias_res_relu", "gate", "res_gate", "leaky", "leaky_gate"]
TILE_OPTION = {64: 0, 128: 2, 256: 1}            # pixel rows per workgroup -> WU_OPT_PW_TILE (option 12)
K_PER_STEP = {"bf16": 64, "fp32": 32}            # channels per 128-byte K step

PwCase = collections.namedtuple("PwCase", "name dtype tile cin cout n hc wc in_stride hin win out_stride hout wout epi seed")


def _pw(dtype, tile, cin, cout, epi, seed, n=1, hc=1, wc=1, in_stride=1, hin=None, win=None, out_stride=1, hout=None, wout=None):
    hin, win = (hc, wc) if hin is None else (hin, win)
    hout, wout = (hc, wc) if hout is None else (hout, wout)
    geo = f"m{n * hc * wc}" if in_stride == 1 and out_stride == 1 else (f"gather{n}x{hin}x{win}" if in_stride == 2 else f"scatter{n}x{hout}x{wout}")
    return PwCase(f"{dtype}-t{tile}-k{cin}-c{cout}-{geo}-{epi}", dtype, tile, cin, cout, n, hc, wc, in_stride, hin, win, out_stride, hout, wout, epi, seed)


# 1445 rows = 22 x 64 + 37 = 11 x 128 + 37 = 5 x 256 + 165: a ragged last tile and many pixel tiles at every tile height, and twelve
# 128-row tiles for the persistent kernel (two items per workgroup on a forced grid of six even with one cout tile)
M_WALK, M_SMALL = 1445, 29


def _pw_cases():
    out, seed = [], 1000
    for dtype in ("bf16", "fp32"):
        for ti, tile in enumerate((64, 128, 256)):
            for steps in range(1, 7):            # every branch of the two-ahead K pipeline at every tile height; every epilogue at every tile height
                seed += 1
                out.append(_pw(dtype, tile, K_PER_STEP[dtype] * steps, 64 if steps % 2 else 192, EPI_ORDER[(steps - 1 + ti) % 6], seed, wc=M_WALK))
    # Cout % 128 == 0: the 128-cout tiles of the persistent kernel (four / eight waves, ring depth 2-4)
    out.append(_pw("bf16", 64, 128, 128, "bias_res_relu", 1101, wc=M_WALK))
    out.append(_pw("bf16", 64, 192, 256, "res_gate", 1102, wc=M_WALK))
    out.append(_pw("bf16", 64, 64, 128, "leaky_gate", 1103, wc=M_WALK))
    out.append(_pw("bf16", 64, 320, 128, "leaky", 1104, wc=M_WALK))
    # fewer rows than one MFMA block
    out.append(_pw("bf16", 64, 64, 64, "bias_res_relu", 1111, wc=M_SMALL))
    out.append(_pw("bf16", 256, 128, 192, "res_gate", 1112, wc=M_SMALL))
    out.append(_pw("fp32", 128, 96, 64, "bias_res_relu", 1113, wc=M_SMALL))
    # stride-2 gather (the downsample conv): input both odd, both even
    for dtype, tile, (hin, win), epi, seed in (("bf16", 64, (9, 7), "bias", 1201), ("bf16", 128, (8, 6), "bias_res_relu", 1202),
                                               ("bf16", 64, (8, 6), "leaky", 1203), ("bf16", 256, (9, 7), "res_gate", 1204),
                                               ("fp32", 64, (9, 7), "bias_res_relu", 1205), ("fp32", 128, (8, 6), "bias", 1206)):
        out.append(_pw(dtype, tile, 128, 64, epi, seed, n=3, hc=(hin - 1) // 2 + 1, wc=(win - 1) // 2 + 1, in_stride=2, hin=hin, win=win))
    # stride-2 scatter (its data gradient): output (2 Hc, 2 Wc) -- the production shape --, (2 Hc - 1, 2 Wc - 1), (2 Hc, 2 Wc - 1)
    hc, wc = 5, 4
    seed = 1300
    for hout, wout in ((2 * hc, 2 * wc), (2 * hc - 1, 2 * wc - 1), (2 * hc, 2 * wc - 1)):
        for dtype, tile, cin, epi in (("bf16", 64, 128, "bare"), ("bf16", 64, 64, "res_gate"), ("bf16", 128, 192, "res_gate"), ("fp32", 64, 96, "res_gate"),
                                      ("fp32", 256, 32, "bare")):
            seed += 1
            out.append(_pw(dtype, tile, cin, 64 if cin != 192 else 192, epi, seed, n=3, hc=hc, wc=wc, out_stride=2, hout=hout, wout=wout))
    return out


PW_CASES = _pw_cases()


def pw_bound(c):
    """Worst-case |sum + bias + residual| of a case (a planted bias cancels a sum: it is at most the sum's own bound)."""
    return 2 * c.cin * PW_RX * PW_RW + RR


def gather_rows(x):
    """in_stride = 2: GEMM row (n, hc, wc) reads pixel (2 hc, 2 wc)."""
    return x[:, :, ::2, ::2]


def scatter_rows(v, hout, wout):
    """out_stride = 2: GEMM row (n, hc, wc) lands on site (2 hc, 2 wc) of the Hout x Wout image; the other sites of its 2 x 2 block that lie
    inside the image receive zero (then residual, activation and gate like every site)."""
    n, c, hc, wc = v.shape
    assert 2 * hc - 1 <= hout <= 2 * hc and 2 * wc - 1 <= wout <= 2 * wc
    out = torch.zeros((n, c, hout, wout), dtype=v.dtype)
    out[:, :, ::2, ::2] = v
    return out


def _pw_linear_no_res(c, x, w, bias, acc):
    xs = gather_rows(x) if c.in_stride == 2 else x
    s = F.conv2d(xs.to(acc), w.to(acc).view(c.cout, c.cin, 1, 1), bias.to(acc) if bias is not None else None)
    return scatter_rows(s, c.hout, c.wout) if c.out_stride == 2 else s


def pw_operands(c):
    """x (N, Cin, Hin, Win) on its own grid, w (Cout, Cin), bias / residual / gate (N, Cout, Hout, Wout) or None.  Every 97th residual
    cancels its sum where that fits bf16, and every 8th bias (fp32: any integer) cancels the sum of its channel's first site, so that
    exact zeros meet the activation also where chance would leave none."""
    has_b, has_r, _, gact = EPILOGUES[c.epi]
    hx, wx = (c.hin, c.win) if c.in_stride == 2 else (c.hc, c.wc)
    x = ints((c.n, c.cin, hx, wx), -PW_RX, PW_RX, c.seed)
    w = ints((c.cout, c.cin), -PW_RW, PW_RW, c.seed + 10000)
    bias = ints((c.cout,), -RB, RB, c.seed + 20000) if has_b else None
    if has_b:
        bias[::8] = -_pw_linear_no_res(c, x, w, None, torch.float32)[0, ::8, 0, 0]
    oshape = (c.n, c.cout, c.hout, c.wout)
    res = gate = None
    if has_r:
        res = ints(oshape, -RR, RR, c.seed + 30000)
        s = _pw_linear_no_res(c, x, w, bias, torch.float32)
        plant = torch.zeros(res.numel(), dtype=torch.bool)
        plant[::97] = True
        plant = plant.view(oshape) & (s.abs() <= RR)
        res = torch.where(plant, -s, res)
    if gact != NONE:
        gate = ints(oshape, -RG, RG, c.seed + 40000)
    return dict(x=x, w=w, bias=bias, res=res, gate=gate)


def pw_reference(c, ops, acc=torch.float32):
    """(value that meets the activation, value that meets the one rounding), both fp32 (N, Cout, Hout, Wout)."""
    _, _, act, gact = EPILOGUES[c.epi]
    lin = _pw_linear_no_res(c, ops["x"], ops["w"], ops["bias"], acc)
    if ops["res"] is not None:
        lin = lin + ops["res"].to(acc)
    lin = lin.float()
    out = act_apply(lin, act)
    if ops["gate"] is not None:
        out = act_gate(out, ops["gate"], gact)
    return lin, out


def pw3_plan(m, cout, opt15, cus):
    """(items, workgroups) of conv1x1_pw3_kernel's pointwise launch (wu_conv1x1_fwd): 128-row tiles x cout tiles of 128 (64 where Cout is
    an odd multiple of 64, one configuration: ring depth 2); two workgroups per CU at ring depth 2, else one."""
    tn = 128 if cout % 128 == 0 else 64
    items = -(-m // 128) * (cout // tn)
    depth = 2 if tn == 64 else opt15 & 7
    return items, min(items, (2 if depth == 2 else 1) * cus)


PW3_OPTIONS = [16 + 2, 16 + 8 + 2, 16 + 4, 16 + 8 + 3]
PW3_FORCED_CUS = 3


def pw3_cases():
    """The stride-1 bf16 cases of PW_CASES with enough rows to be walked on the forced grid, and the ones below one MFMA block."""
    s1 = [c for c in PW_CASES if c.dtype == "bf16" and c.in_stride == 1 and c.out_stride == 1]
    return [c for c in s1 if c.wc == M_WALK], [c for c in s1 if c.wc == M_SMALL]


# ---------------------------------------------------------------------------------------------------------------------------------
# conv1x1_chain_kernel: two GEMMs, the ROUNDED y1 feeds the second
# ---------------------------------------------------------------------------------------------------------------------------------
ChainCase = collections.namedtuple("ChainCase", "name form k1 c1 c2 m seed")
CHAIN_RWB = 1
CHAIN_ZERO_ROW = 7           # row of wb (and entry of bias_b) that is zero: exact zeros in front of the second activation at any size
CHAIN_CASES = [ChainCase(f"{form}-k{k1}-c{c1}-c{c2}-m{m}", form, k1, c1, c2, m, 2000 + i)
               for i, (form, (k1, c1, c2, m)) in enumerate((f, s) for f in ("forward", "backward")
                                                           for s in ((64, 256, 32, 5), (128, 512, 64, 37), (256, 1024, 160, 70), (256, 256, 160, 37), (64, 1024, 64, 70)))]


def chain_bounds(c):
    """Worst-case |pre-activation| of stage 1 and of stage 2 (whose operand is the bf16-rounded y1: at most one part in 256 larger)."""
    b1 = c.k1 * RX * RW + RB + RR
    return b1, c.c1 * (b1 + b1 // 256 + 1) * CHAIN_RWB + RB


def chain_operands(c):
    shp = lambda ch: (1, ch, 1, c.m)      # noqa: E731
    fwd = c.form == "forward"
    x = ints(shp(c.k1), -RX, RX, c.seed)
    wa = ints((c.c1, c.k1), -RW, RW, c.seed + 10000)
    wb = ints((c.c2, c.c1), -CHAIN_RWB, CHAIN_RWB, c.seed + 20000)
    wb[CHAIN_ZERO_ROW] = 0
    bias_a = ints((c.c1,), -RB, RB, c.seed + 30000) if fwd else None
    bias_b = ints((c.c2,), -RB, RB, c.seed + 40000) if fwd else None
    if fwd:
        bias_b[CHAIN_ZERO_ROW] = 0
    res = ints(shp(c.c1), -RR, RR, c.seed + 50000)
    s = F.conv2d(x, wa.view(c.c1, c.k1, 1, 1), bias_a)
    plant = torch.zeros(res.numel(), dtype=torch.bool)
    plant[::97] = True
    plant = plant.view(res.shape) & (s.abs() <= RR)
    res = torch.where(plant, -s, res)
    gate1 = None if fwd else ints(shp(c.c1), -RG, RG, c.seed + 60000)
    gate2 = None if fwd else ints(shp(c.c2), -RG, RG, c.seed + 70000)
    return dict(x=x, wa=wa, wb=wb, bias_a=bias_a, bias_b=bias_b, res=res, gate1=gate1, gate2=gate2)


def chain_reference(c, ops, acc=torch.float32):
    """(lin1, y1, lin2, y2) in fp32; forward: bias + residual + ReLU, then bias + ReLU; backward: residual + ReLU gate, then ReLU gate."""
    fwd = c.form == "forward"
    b = lambda t: t.to(acc) if t is not None else None      # noqa: E731
    lin1 = (F.conv2d(ops["x"].to(acc), ops["wa"].to(acc).view(c.c1, c.k1, 1, 1), b(ops["bias_a"])) + ops["res"].to(acc)).float()
    y1 = act_apply(lin1, RELU) if fwd else act_gate(lin1, ops["gate1"], RELU)
    y1r = y1.bfloat16().float()          # what the kernel stores AND what its second GEMM reads: still integers
    lin2 = F.conv2d(y1r.to(acc), ops["wb"].to(acc).view(c.c2, c.c1, 1, 1), b(ops["bias_b"])).float()
    y2 = act_apply(lin2, RELU) if fwd else act_gate(lin2, ops["gate2"], RELU)
    return lin1, y1, lin2, y2


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 x 3 stride-2 conv and its data gradient (conv1x1_pw3_kernel<.., CONV> and the kernels it replaces)
# ---------------------------------------------------------------------------------------------------------------------------------
S2Case = collections.namedtuple("S2Case", "name n cin cout h w seed walked")
# walked: enough 128-row tiles that every workgroup of the forced grid (2 x 3) owns at least two items, forward and backward
S2_CASES = [S2Case(f"{n}x{cin}x{cout}x{h}x{w}", n, cin, cout, h, w, 3000 + i, walked)
            for i, (n, cin, cout, h, w, walked) in enumerate(((2, 64, 64, 2, 2, False), (3, 64, 128, 5, 7, False), (1, 128, 64, 11, 13, False),
                                                              (2, 128, 128, 12, 10, False), (2, 64, 192, 9, 8, False), (3, 64, 128, 118, 16, True)))]
S2_GATHERED, S2_FORCED_CUS = 16 + 2 + 8, 3       # option 15 of the gathered-row form (64-cout tiles allowed); option 10 of its small grid
S2_FWD_EPILOGUES = {"bias_leaky": (LEAKY, NONE), "bias_relu_gate": (RELU, RELU)}
S2_DGRAD_EPILOGUES = {"ungated": NONE, "leaky_gated": LEAKY}
S2_RX, S2_RW = 16, 8         # a 2 x 2 image has one tap per site in its data gradient: 64 products must be able to leave bf16
S2_ZERO_CHANNEL = 5          # input channel whose weights are zero: its data gradient is exactly zero at any size


def s2_bounds(c):
    """Forward (the planted bias cancels a sum: up to the sum's own bound) and data gradient."""
    return 2 * 9 * c.cin * S2_RX * S2_RW, 9 * c.cout * S2_RX * S2_RW


def s2_operands(c):
    ho, wo = (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
    x = ints((c.n, c.cin, c.h, c.w), -S2_RX, S2_RX, c.seed)
    w = ints((c.cout, c.cin, 3, 3), -S2_RW, S2_RW, c.seed + 10000)
    w[:, S2_ZERO_CHANNEL] = 0
    bias = ints((c.cout,), -RB, RB, c.seed + 20000)
    s = F.conv2d(x, w, None, stride=2, padding=1)
    bias[::8] = -s[0, ::8, 0, 0]         # every 8th channel: an exact zero at the first output site, whatever the image size
    gate = ints((c.n, c.cout, ho, wo), -RG, RG, c.seed + 30000)
    dy = ints((c.n, c.cout, ho, wo), -S2_RX, S2_RX, c.seed + 40000)
    xgate = ints((c.n, c.cin, c.h, c.w), -RG, RG, c.seed + 50000)
    return dict(x=x, w=w, bias=bias, gate=gate, dy=dy, xgate=xgate)


def s2_forward_reference(c, ops, epi, acc=torch.float32):
    act, gact = S2_FWD_EPILOGUES[epi]
    lin = F.conv2d(ops["x"].to(acc), ops["w"].to(acc), ops["bias"].to(acc), stride=2, padding=1).float()
    out = act_apply(lin, act)
    return lin, (act_gate(out, ops["gate"], gact) if gact != NONE else out)


def s2_dgrad_reference(c, ops, epi, acc=torch.float32):
    lin = torch.nn.grad.conv2d_input((c.n, c.cin, c.h, c.w), ops["w"].to(acc), ops["dy"].to(acc), stride=2, padding=1).float()
    gact = S2_DGRAD_EPILOGUES[epi]
    return lin, (act_gate(lin, ops["xgate"], gact) if gact != NONE else lin)


def pw3_conv_plan(m, cout, ncls, cus):
    """(items, workgroups) of the gathered-row launches (pw3_conv_launch): 128-row tiles x cout tiles x parity classes on 2 x CUs."""
    tn = 128 if cout % 128 == 0 else 64
    items = -(-m // 128) * (cout // tn) * ncls
    return items, min(items, 2 * cus)


# ---------------------------------------------------------------------------------------------------------------------------------
# stem: conv 7 x 7, stride 2, pad 3, 3 -> 64 from the NCHW fp32 image, and its data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
StemCase = collections.namedtuple("StemCase", "name n h w act seed")
STEM_FWD_CASES = [StemCase(f"{n}x{h}x{w}-{'relu' if act == RELU else 'none'}", n, h, w, act, 4000 + i)
                  for i, (n, h, w, act) in enumerate((n, h, w, a) for (n, h, w) in ((2, 7, 7), (3, 20, 36), (2, 33, 70), (2, 16, 130)) for a in (RELU, NONE))]
STEM_RX, STEM_RW = 16, 8       # the corner windows of a 7 x 7 image hold 16 of the 49 taps
STEM_TH, STEM_TW = 8, 32             # output pixels per tile of both forward kernels
DGRAD_TH, DGRAD_TW = 16, 32          # input pixels per tile of stem7x7_dgrad_mfma_kernel
StemDgradCase = collections.namedtuple("StemDgradCase", "name kind n h w seed")
# kind: which kernel wu_stem7x7_dgrad picks -- bf16 with even sizes: the matrix-core kernel; bf16 with an odd size and fp32: the VALU kernel
STEM_DGRAD_CASES = [StemDgradCase(f"{kind}-{n}x{h}x{w}", kind, n, h, w, 5000 + i)
                    for i, (kind, n, h, w) in enumerate((("mfma", 3, 8, 8), ("mfma", 2, 34, 66), ("valu_bf16", 2, 7, 9), ("valu_bf16", 2, 33, 35),
                                                         ("valu_bf16", 2, 34, 35), ("fp32", 2, 8, 8), ("fp32", 2, 33, 35)))]


def stem_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def stem_fwd_tiles(c):
    ho, wo = stem_out(c.h, c.w)
    return c.n * -(-ho // STEM_TH) * -(-wo // STEM_TW)


def stem_dgrad_tiles(c):
    return c.n * -(-c.h // DGRAD_TH) * -(-c.w // DGRAD_TW)


def stem_bounds():
    """Forward: 147 products + bias (a planted bias cancels a sum: at most the sum's own bound).  Data gradient: at most 4 x 4 taps x 64 channels reach an input pixel; + the accumulated integer."""
    return 2 * 147 * STEM_RX * STEM_RW, 16 * 64 * STEM_RX * STEM_RW + 5


def stem_operands(c):
    x = ints((c.n, 3, c.h, c.w), -STEM_RX, STEM_RX, c.seed)
    w = ints((64, 3, 7, 7), -STEM_RW, STEM_RW, c.seed + 10000)
    bias = ints((64,), -RB, RB, c.seed + 20000)
    bias[::8] = -F.conv2d(x, w, None, stride=2, padding=3)[0, ::8, 0, 0]     # exact zeros in front of the activation at any size
    return dict(x=x, w=w, bias=bias)


def stem_forward_reference(c, ops, acc=torch.float32):
    lin = F.conv2d(ops["x"].to(acc), ops["w"].to(acc), ops["bias"].to(acc), stride=2, padding=3).float()
    return lin, act_apply(lin, c.act)


def stem_dgrad_operands(c):
    ho, wo = stem_out(c.h, c.w)
    dy = ints((c.n, 64, ho, wo), -STEM_RX, STEM_RX, c.seed)
    w = ints((64, 3, 7, 7), -STEM_RW, STEM_RW, c.seed + 10000)
    dx0 = ints((c.n, 3, c.h, c.w), -5, 5, c.seed + 20000)
    return dict(dy=dy, w=w, dx0=dx0)


def stem_dgrad_reference(c, ops, acc=torch.float32):
    """dx of F.conv2d(x, w, stride 2, pad 3) for the output gradient dy, through autograd."""
    x = torch.zeros((c.n, 3, c.h, c.w), dtype=acc, requires_grad=True)
    F.conv2d(x, ops["w"].to(acc), None, stride=2, padding=3).backward(ops["dy"].to(acc))
    return x.grad.float()
