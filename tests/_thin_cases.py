"""Case tables of tests/test_gpu_thin_exact.py: shapes, value ranges with their worst-case sums, and for every row the kernel of
csrc/thin.hip it was written for.  tests/test_thin_ref_cpu.py checks, without a GPU, that every bound satisfies the oracle's premise and
that the dispatch restatement of tests/_thin_ref.py names that kernel."""
from _thin_ref import BF16, F32, out_hw

# single pixels, single rows / columns, 32-pixel blocks spanning rows and images, all four H/W parities at stride 2, exact and ragged
# 8 x 32 and 16 x 64 tiles, two tiles in x and y
E = [(1, 1, 1), (3, 1, 1), (1, 2, 2), (1, 1, 70), (1, 70, 1), (3, 5, 7), (2, 16, 64), (1, 15, 63), (2, 17, 19), (2, 33, 66), (1, 34, 130)]
# name -> ((N, H, W), stride): more than one iteration per wave of the 3 -> 64 matrix-core forward (> 524288 output pixels)
L = {"L1": ((2, 512, 520), 1),         # 532480 pixels, % 32 == 0: 16640 blocks over 16384 waves
     "L1x": ((4, 512, 520), 1),        # some waves run three iterations
     "L2": ((3, 419, 421), 1),         # 529197 pixels, % 32 == 13: the non-FULL instance
     "L3": ((8, 520, 512), 2),         # 260 x 256 outputs, FULL
     "L4": ((8, 521, 515), 2)}         # 261 x 258 outputs, 538704 pixels, non-FULL

XMAX, WMAX, BMAX, GMAX, GMAX_LEAKY, ISG_MAX, PRELOAD = 4, 2, 8, 2, 10, 2, 8
INV_SIGMAS = (None, 0.5, 2.0)


def npix(shape, stride=1):
    n, h, w = shape
    ho, wo = out_hw(h, w, stride)
    return n * ho * wo


def fwd_bound():
    return 27 * XMAX * WMAX * ISG_MAX + BMAX


def wgrad_xmax(shape, stride, gmax):
    """The widest image range whose weight-gradient sum keeps the oracle's premise: |x| <= 4, narrowed to 2 or 1 where needed."""
    for xm in (XMAX, 2, 1):
        if wgrad_bound(shape, stride, gmax, xm) < 2 ** 24:
            return xm
    raise AssertionError(f"{shape}: no image range keeps the weight gradient below 2^24")


def wgrad_bound(shape, stride, gmax, xmax):
    return npix(shape, stride) * xmax * gmax + PRELOAD


def dgrad_bound(cout, gmax):
    return 9 * cout * gmax * WMAX * ISG_MAX + PRELOAD


def head_bwd_bound(shape, cin=64):
    """g = dout (1 - out^2) with dout a multiple of 4 in [-8, 8] and out in {0, +-0.5}: an integer, |g| <= 8."""
    n, h, w = shape
    return max(n * h * w * 8 * XMAX, 3 * 8 * WMAX) + PRELOAD


# ---- 3 -> 64 forward: (shape, stride, dtype, WU_OPT_C3_ROWS, bias address mod 16, kernel) ----
FWD64 = ([(s, st, BF16, 0, 0, "conv3x3_c3_fwd_mfma_kernel") for s in E for st in (1, 2)]
         + [(L[k][0], L[k][1], BF16, 0, 0, "conv3x3_c3_fwd_mfma_kernel") for k in L]
         + [(s, st, BF16, 0, 4, "conv3x3_c3_fwd_kernel") for s in E for st in (1, 2)]
         + [(s, st, F32, 0, 0, "conv3x3_c3_fwd_kernel") for s in E for st in (1, 2)]
         + [(s, st, dt, 1, 0, "conv3x3_c3_fwd_rows_kernel") for s in E for st in (1, 2) for dt in (BF16, F32)]
         + [(L["L2"][0], 1, BF16, 1, 0, "conv3x3_c3_fwd_rows_kernel")]
         + [(s, st, BF16, 2, 0, "conv3x3_c3_fwd_kernel") for s in E for st in (1, 2)])

# ---- 3 -> 3 image conv: (shape, WU_OPT_IMG3_TILED, forward kernel, data-gradient kernel) ----
IMG3_SHAPES = E + [(2, 37, 131), (1, 16, 128), (3, 5, 4)]
IMG3 = ([(s, 1, "img3_conv_kernel", "img3_conv_kernel") for s in IMG3_SHAPES]
        + [(s, 0, "conv3x3_c3_fwd_kernel", "conv3x3_c3_dgrad_kernel") for s in IMG3_SHAPES])

# ---- weight gradients: (shape, stride, dtype, dy NCHW, Cout, lddy, WU_OPT_IMG3_TILED, kernel) ----
WGRAD_MFMA = ([(s, st, BF16, False, 64, 192, 1, "conv3x3_c3_wgrad_mfma_kernel") for s in E for st in (1, 2)]
              + [(L[k][0], L[k][1], BF16, False, 64, 192, 1, "conv3x3_c3_wgrad_mfma_kernel") for k in ("L1", "L2", "L4")])
WGRAD_GENERIC_SHAPES = E + [(2, 200, 200)]           # 80000 pixels exceed the 1024 x 64 grid
WGRAD_GENERIC = ([(s, st, F32, False, 64, 192, 1, "conv3x3_c3_wgrad_kernel") for s in WGRAD_GENERIC_SHAPES for st in (1, 2)]
                 + [(s, st, BF16, False, 64, 68, 1, "conv3x3_c3_wgrad_kernel") for s in WGRAD_GENERIC_SHAPES for st in (1, 2)]
                 # pixel stride 76 from channel 8: the ADDRESS is 16-byte aligned, only the stride is not
                 + [(s, st, BF16, False, 64, 76, 1, "conv3x3_c3_wgrad_kernel") for s in E for st in (1, 2)])
IMG3_WGRAD_SHAPES = E + [(3, 176, 2048)]             # 11 x 32 x 3 = 1056 tiles exceed the 1024-workgroup cap
IMG3_WGRAD = [(s, 1, F32, True, 3, 0, 1, "img3_wgrad_kernel") for s in IMG3_WGRAD_SHAPES]
WGRAD_SMALL_SHAPES = E + [(2, 364, 364)]             # 264992 pixels exceed the 1024 x 256 grid
WGRAD_SMALL = ([(s, 1, F32, True, 3, 0, 0, "conv3x3_c3_wgrad_small_kernel") for s in WGRAD_SMALL_SHAPES]
               + [(s, 2, F32, True, 3, 0, 1, "conv3x3_c3_wgrad_small_kernel") for s in WGRAD_SMALL_SHAPES]
               + [(s, st, F32, True, co, 0, 1, "conv3x3_c3_wgrad_small_kernel") for s in WGRAD_SMALL_SHAPES for st in (1, 2) for co in (1, 2)])

# ---- data gradients: (shape, stride, dtype, dy NCHW, Cout, lddy, y address mod 16 (None: no gate), ldy, kernel) ----
DGRAD_S2 = [(s, 2, BF16, False, 64, 192, ym, 192, "conv3x3_c3_dgrad_s2_mfma_kernel") for s in E for ym in (None, 0)]
DGRAD_NHWC_SHAPES = E + [(2, 260, 256)]              # 133120 input pixels exceed both grid caps (4096 x 32 and 4096 x 16)
DGRAD_NHWC = ([(s, 1, BF16, False, 64, 192, ym, 192, "conv3x3_c3_dgrad_nhwc_kernel") for s in DGRAD_NHWC_SHAPES for ym in (None, 0)]
              + [(s, st, F32, False, 64, 192, ym, 192, "conv3x3_c3_dgrad_nhwc_kernel") for s in DGRAD_NHWC_SHAPES for st in (1, 2) for ym in (None, 0)]
              # bf16 at stride 2 reaches this kernel only for Cout != 64 (the matrix-core kernel takes every aligned 64-channel call)
              + [(s, 2, BF16, False, 32, 192, ym, 192, "conv3x3_c3_dgrad_nhwc_kernel") for s in E for ym in (None, 0)])
# a gate tensor that is not 16-byte aligned fails the alignment test of BOTH kernels above: the call falls through to the generic kernel
DGRAD_GENERIC = ([(s, 2, BF16, False, 64, 192, 4, 68, "conv3x3_c3_dgrad_kernel") for s in E]
                 + [(s, st, BF16, False, 64, 68, None, 0, "conv3x3_c3_dgrad_kernel") for s in E for st in (1, 2)]
                 + [(s, st, BF16, False, 64, 76, None, 0, "conv3x3_c3_dgrad_kernel") for s in E for st in (1, 2)]      # aligned address, unaligned stride
                 + [(s, st, F32, True, 3, 0, 0, 0, "conv3x3_c3_dgrad_kernel") for s in E for st in (1, 2)]
                 + [((8, 520, 512), 1, F32, True, 3, 0, 0, 0, "conv3x3_c3_dgrad_kernel")])     # 2.13 M pixels exceed the 8192 x 256 grid

# ---- tanh head ----
HEAD_BWD_SHAPES = [(1, 1, 1), (2, 12, 20), (3, 5, 7), (2, 130, 127)]      # 33020 pixels: both dtypes loop, with a ragged tail
HEAD_FWD_SHAPES = [(2, 12, 20), (1, 1, 1), (3, 5, 7), (64, 65, 65)]       # 4225 pixels per image on a 64-workgroup cap: a loop and a tail
HEAD_FWD_CIN = {BF16: (32, 64, 128, 512), F32: (16, 64, 256)}             # lanes per pixel 4, 8, 16, 64 and 4, 16, 64
