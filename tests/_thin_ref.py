"""CPU oracle of the thin-layer kernels (csrc/thin.hip): the 3 -> 64 and 3 -> 3 image convs, their gradients, the 64 -> 3 tanh head.

Plain torch / numpy in fp64; nothing of the library is imported.  On small INTEGER operands (and a power-of-two inv_sigma) every sum
is an integer below 2^24, so fp32 addition is exact in any order and the matrix-core, VALU, atomic and slab-fold paths must all give
the bits computed here: `exact(bound)` is that premise, asserted per case with the case's own worst-case sum.  LeakyReLU is ONE fp32
multiply by float32(0.2) (v <= 0 forward, y <= 0 in a gate): the fp64 product of two fp32 values is exact, so rounding it to fp32 once
is that multiply.  float32(0.2) * 5k rounds to k exactly (tests/test_thin_ref_cpu.py), hence gradients under a Leaky gate are drawn from
multiples of 5 and the re-rounding to bf16 of the matrix-core paths changes nothing.

`real=True` keeps everything in fp64 with slope 0.2 and asserts nothing about exactness: that form is compared with torch autograd on
random real inputs, so the oracle is not its own reference.

The second half restates the host dispatch of c3_fwd_impl, wu_conv3x3_c3_wgrad and wu_conv3x3_c3_dgrad: which kernel a call reaches."""
import numpy as np
import torch
import torch.nn.functional as F

NONE, RELU, LEAKY = 0, 1, 2            # WU_ACT_* (include/wu_kernels.h)
F32, BF16 = 0, 1                       # WU_F32 / WU_BF16
SLOPE32 = float(np.float32(0.2))       # the fp32 constant 0.2f as a double


def ints(shape, lo, hi, seed, step=1):
    """Seeded integers in [lo, hi] that are multiples of `step`, as fp32."""
    assert lo % step == 0 and hi % step == 0
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo // step, hi // step + 1, tuple(shape), generator=g) * step).float()


def exact(bound):
    """The premise of the oracle: every partial sum is an integer below 2^24, so fp32 addition is exact in any order."""
    assert bound < 2 ** 24, f"integer oracle out of range: worst-case sum {bound} >= 2^24"


def _f32_exact(v64, what):
    v32 = v64.float()
    assert torch.equal(v32.double(), v64), f"{what}: not representable in fp32 (the integer premise is broken)"
    return v32


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def act_apply(v64, act, real=False):
    """fp64 in; fp32 out (fp64 when real): ReLU is max(v, 0), LeakyReLU one fp32 multiply by float32(0.2) for v <= 0."""
    if act == RELU:
        r = torch.clamp_min(v64, 0.0)
    elif act == LEAKY:
        r = torch.where(v64 > 0, v64, v64 * (0.2 if real else SLOPE32))
    else:
        r = v64
    return r if real else r.float()


def act_gate(g, y, act, real=False):
    """g where y > 0; otherwise 0 (ReLU) or float32(0.2) * g (Leaky).  fp64 out."""
    g, y = g.double(), y.double()
    if act == RELU:
        return torch.where(y > 0, g, torch.zeros_like(g))
    if act == LEAKY:
        low = g * 0.2 if real else (g * SLOPE32).float().double()
        return torch.where(y > 0, g, low)
    return g


def conv_fwd(x, w, b, inv_sigma, stride, act, real=False):
    """(y, gate bits): y = act(conv3x3(x, w * inv_sigma, pad 1) + b) as fp32 (a bf16 kernel stores y.bfloat16(), round to nearest
    even), bits = (y > 0)."""
    s = 1.0 if inv_sigma is None else float(inv_sigma)
    pre = F.conv2d(x.double(), w.double() * s, b.double() if b is not None else None, stride=stride, padding=1)
    if not real:
        _f32_exact(pre, "pre-activation")
    y = act_apply(pre, act, real)
    return y, y > 0


def conv_wgrad(x, dy, y, act, stride, real=False):
    """(dW [Cout, 3, 3, 3], db [Cout]) of the conv above from the gated output gradient (y None: ungated)."""
    g = act_gate(dy, y, act, real) if y is not None else dy.double()
    n, cout = g.shape[:2]
    cols = F.unfold(x.double(), 3, padding=1, stride=stride)                    # (N, 27, Ho * Wo), k = ci * 9 + kh * 3 + kw
    dw = torch.einsum("ncl,nkl->ck", g.reshape(n, cout, -1), cols).reshape(cout, 3, 3, 3)
    db = g.sum(dim=(0, 2, 3))
    return (dw, db) if real else (_f32_exact(dw, "dW"), _f32_exact(db, "db"))


def conv_dgrad(dy, y, act, w, inv_sigma, stride, H, W, real=False):
    """dx [N, 3, H, W] of the conv above from the gated output gradient."""
    g = act_gate(dy, y, act, real) if y is not None else dy.double()
    s = 1.0 if inv_sigma is None else float(inv_sigma)
    ho, wo = g.shape[2:]
    assert (ho, wo) == out_hw(H, W, stride)
    op = (H - 1 - (ho - 1) * stride, W - 1 - (wo - 1) * stride)
    dx = F.conv_transpose2d(g, w.double() * s, stride=stride, padding=1, output_padding=op)
    assert dx.shape[2:] == (H, W)
    return dx if real else _f32_exact(dx, "dx")


def tanh_head_bwd(dout, out, x, w, x_gate_act, real=False):
    """Backward of out = tanh(conv1x1(x, w [3, Cin]) + b): g = dout (1 - out^2); dx = gate(sum_k g_k w_k, x); dW = sum_pix g (x) x;
    db = sum_pix g."""
    g = dout.double() * (1.0 - out.double() * out.double())
    dx = act_gate(torch.einsum("nkhw,kc->nchw", g, w.double()), x, x_gate_act, real)
    dw = torch.einsum("nkhw,nchw->kc", g, x.double())
    db = g.sum(dim=(0, 2, 3))
    return (dx, dw, db) if real else (_f32_exact(dx, "head dx"), _f32_exact(dw, "head dW"), _f32_exact(db, "head db"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the host dispatch of csrc/thin.hip, restated: the kernel a call is meant to reach
# ---------------------------------------------------------------------------------------------------------------------------------
I3H, I3W = 16, 64                      # kI3H, kI3W: the tile of the LDS-tiled 3 -> 3 kernels


def _img3_ok(n, h, w):
    return n * -(-h // I3H) * -(-w // I3W) < 2 ** 31


def _aligned(ptr_mod16, ld, esz):
    return ptr_mod16 == 0 and (ld * esz) % 16 == 0


def fwd_kernel(dtype, out_nchw, n, h, w, cout, stride, bias_mod16=0, c3_rows=0, img3_tiled=1):
    """c3_fwd_impl.  bias_mod16: the bias address modulo 16 (None: no bias)."""
    ho, wo = out_hw(h, w, stride)
    if out_nchw:
        return "img3_conv_kernel" if img3_tiled and _img3_ok(n, h, w) else "conv3x3_c3_fwd_kernel"
    mfma = (dtype == BF16 and cout == 64 and c3_rows == 0 and (bias_mod16 is None or bias_mod16 == 0)
            and n * ho * wo < 2 ** 31 - 64 and n * 3 * h * w < 2 ** 28)
    if mfma:
        return "conv3x3_c3_fwd_mfma_kernel"
    return "conv3x3_c3_fwd_rows_kernel" if c3_rows == 1 else "conv3x3_c3_fwd_kernel"


def wgrad_kernel(dtype, dy_nchw, n, h, w, cout, stride, dy_mod16=0, lddy=64, y_mod16=None, ldy=64, img3_tiled=1):
    """wu_conv3x3_c3_wgrad.  y_mod16 None: no gate tensor."""
    ho, wo = out_hw(h, w, stride)
    mfma = (not dy_nchw and dtype == BF16 and cout == 64 and n * ho * wo < 2 ** 31 and n * 3 * h * w < 2 ** 28
            and dy_mod16 == 0 and lddy % 8 == 0 and (y_mod16 is None or (y_mod16 == 0 and ldy % 8 == 0)))
    if mfma:
        return "conv3x3_c3_wgrad_mfma_kernel"
    if dy_nchw and cout == 3 and stride == 1 and img3_tiled and _img3_ok(n, h, w):
        return "img3_wgrad_kernel"
    if dy_nchw and cout <= 3:
        return "conv3x3_c3_wgrad_small_kernel"
    return "conv3x3_c3_wgrad_kernel"


def dgrad_kernel(dtype, dy_nchw, n, h, w, cout, stride, dy_mod16=0, lddy=64, y_mod16=None, ldy=64, img3_tiled=1):
    """wu_conv3x3_c3_dgrad."""
    esz = 2 if dtype == BF16 else 4
    per16 = 16 // esz
    y_ok8 = y_mod16 is None or (y_mod16 == 0 and ldy % 8 == 0)
    if not dy_nchw and dtype == BF16 and stride == 2 and cout == 64 and dy_mod16 == 0 and lddy % 8 == 0 and y_ok8:
        ho, wo = out_hw(h, w, 2)
        if n * -(-wo // 32) * -(-ho // 8) < 2 ** 31:
            return "conv3x3_c3_dgrad_s2_mfma_kernel"
    lp = 0 if dy_nchw else cout // per16
    if (not dy_nchw and n * h * w < 2 ** 32 and cout % per16 == 0 and 1 <= lp <= 64 and lp & (lp - 1) == 0 and _aligned(dy_mod16, lddy, esz)
            and (y_mod16 is None or _aligned(y_mod16, ldy, esz))):
        return "conv3x3_c3_dgrad_nhwc_kernel"
    if dy_nchw and cout == 3 and stride == 1 and y_mod16 is None and img3_tiled and _img3_ok(n, h, w):
        return "img3_conv_kernel"
    return "conv3x3_c3_dgrad_kernel"


# the grid caps hard-coded in csrc/thin.hip: the pixel counts above which a prefetch / grid-stride loop runs a second iteration
FWD_MFMA_LOOP_PIXELS = 4096 * 4 * 32          # grid_cap(.., 128, 256 * 16) workgroups x 4 waves x 32 pixels
WGRAD_MFMA_LOOP_PIXELS = 1024 * 256           # kThinMaxBlocks workgroups x 256-pixel tiles
ROWS_LOOP_PIXELS = 2048 * 256                 # grid_cap(.., 256, 256 * 8) x 256
WGRAD_GENERIC_LOOP_PIXELS = 1024 * 64
WGRAD_SMALL_LOOP_PIXELS = 1024 * 256
IMG3_WGRAD_LOOP_TILES = 1024
DGRAD_GENERIC_LOOP_PIXELS = 8192 * 256
DGRAD_NHWC_LOOP_GROUPS = 4096                 # grid_cap(.., 256 / LP, 256 * 16) workgroups of 256 / LP pixels
TANH_BWD_LOOP_GROUPS = 1024
