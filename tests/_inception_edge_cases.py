"""The cases of tests/test_gpu_inception_edges.py: the exact small-integer oracle of the InceptionV3 implicit-GEMM conv (conv_kxk_kernel,
csrc/inception.hip) and the stress rows of the feature statistics.  Everything here is CPU work in int64 / float64 on small tensors and
imports nothing of the HIP library.

Every conv case is ASSERTED at import to tell a right kernel from the named wrong ones: its expected output differs, in the stored dtype, from
the output of a kernel with the pads swapped, the weight's kh / kw axes transposed, the batch read as one tall image (or its rows read as one
long row), or the K tail of the last step dropped -- wherever that variant applies to the case.  A case that stops discriminating fails at
collection instead of passing for nothing (the pattern of tests/_gif_enc_cases.py).

Operands are integers: activations in [-4, 4], weights in [-2, 2], bias in [-8, 8], all exact in bf16.  With K <= 4032 every partial sum
stays below 4032 * 8 + 8 < 2^24, so fp32 accumulation is exact in ANY order and the only rounding is the epilogue's store."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU = 0, 1
KE = {"fp32": 32, "bf16": 64}                 # K elements per 128-byte step
TM = 128                                      # output pixels per workgroup
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16}
SENTINEL = -77.0                              # exact in bf16; fills the output buffer around (and under) the written slice
FILL = 3.0                                    # the input buffer's channels outside the slice the conv may read

# x_off / y_off: channel offset of the slice inside a pixel of ldx / ldy channels (8 elements = 16 bytes in bf16, 32 in fp32)
ConvCase = namedtuple("ConvCase", "name n h w cin cin_w cout k s p act x_off ldx y_off ldy seed")
CONV_CASES = {}
_expected = {}


def out_hw(c):
    return (c.h + 2 * c.p[0] - c.k[0]) // c.s + 1, (c.w + 2 * c.p[1] - c.k[1]) // c.s + 1


def operands(c):
    """(x int64 (N, Cin, H, W), w int64 (Cout, Cin_w, KH, KW), bias int64 (Cout,)).  x carries values in ALL Cin channels: the packed weight
    is zero for the channels >= Cin_w, so what the activations hold there must not matter."""
    g = torch.Generator().manual_seed(c.seed)
    x = torch.randint(-4, 5, (c.n, c.cin, c.h, c.w), generator=g)
    w = torch.randint(-2, 3, (c.cout, c.cin_w, c.k[0], c.k[1]), generator=g)
    b = torch.randint(-8, 9, (c.cout,), generator=g)
    return x, w, b


def k_tail(c, prec):
    """K elements of the last, partly filled step (0: K is a whole number of steps)."""
    return (c.k[0] * c.k[1] * c.cin) % KE[prec]


def _reference(c, variant=None, prec=None):
    """float64 output (N, Cout, Ho, Wo) of the conv, or of the named wrong kernel, on the grid the host computes from the TRUE pads."""
    x, w, b = operands(c)
    x, w, b = x[:, :c.cin_w].double(), w.double(), b.double()
    ho, wo = out_hw(c)
    ph, pw = c.p
    kh, kw = c.k
    if variant == "kdrop":
        # k = (kh * KW + kw) * Cin + ci over the PADDED channel count: zero the weights of the last K mod KE positions
        k0 = kh * kw * c.cin - k_tail(c, prec)
        kidx = (torch.arange(kh * kw).view(kh, kw, 1) * c.cin + torch.arange(c.cin_w).view(1, 1, -1)).permute(2, 0, 1)
        w = w * (kidx < k0).double()
    if variant == "transpose":
        w = w.transpose(2, 3)
    if variant == "pads_swapped":
        # ih = oh - pw + kh, iw = ow - ph + kw on the Ho x Wo grid: a window of the conv over a generously zero-padded input
        assert c.s == 1
        q = max(kh, kw)
        full = F.conv2d(F.pad(x, (q, q, q, q)), w, b, 1, 0)
        y = full[:, :, q - pw:q - pw + ho, q - ph:q - ph + wo]
    elif variant == "tall":
        # no zero rows between images: image n + 1 starts where image n ends
        assert c.s == 1 and ho == c.h
        y = F.conv2d(x.permute(1, 0, 2, 3).reshape(1, c.cin_w, c.n * c.h, c.w), w, b, 1, c.p)
        y = y.view(c.cout, c.n, ho, wo).permute(1, 0, 2, 3)
    elif variant == "long_row":
        # no zero columns between rows: the flat pixel index simply runs on (1 x KW kernels)
        assert c.s == 1 and kh == 1 and wo == c.w
        y = F.conv2d(x.permute(1, 0, 2, 3).reshape(1, c.cin_w, 1, c.n * c.h * c.w), w, b, 1, c.p)
        y = y.view(c.cout, c.n, ho, wo).permute(1, 0, 2, 3)
    else:
        y = F.conv2d(x, w, b, c.s, c.p)
    assert tuple(y.shape) == (c.n, c.cout, ho, wo)
    return F.relu(y) if c.act == ACT_RELU else y


def _store(y, prec):
    """The epilogue's one rounding: float32 (exact here), then bf16 round-to-nearest-even."""
    y = y.to(torch.float32)
    return y if prec == "fp32" else y.to(torch.bfloat16)


def expected(name, prec):
    """Expected output in the stored dtype, computed once."""
    if (name, prec) not in _expected:
        _expected[name, prec] = _store(_reference(CONV_CASES[name]), prec)
    return _expected[name, prec]


def variants(c, prec):
    """The wrong kernels this case must tell from the right one."""
    (kh, kw), (ph, pw) = c.k, c.p
    v = []
    if ph != pw:
        v.append("pads_swapped")
    if kh == kw and kh > 1:
        v.append("transpose")
    if ph > 0:
        v.append("tall")
    if kh == 1 and pw > 0:
        v.append("long_row")
    if k_tail(c, prec):
        v.append("kdrop")
    return v


def branch(c, prec):
    """Which path of wu_conv_kxk_fwd / conv_kxk_kernel the case takes (for the log and the case table's own asserts)."""
    ho, wo = out_hw(c)
    m = c.n * ho * wo
    cout32 = -(-c.cout // 32) * 32
    ni = 2 if cout32 % 64 == 0 else 1
    k = c.k[0] * c.k[1] * c.cin
    return {"instance": f"conv_kxk_kernel<{prec}, {ni}>", "ni": ni, "cout_tiles": cout32 // (32 * ni), "masked_couts": cout32 - c.cout,
            "M": m, "pixel_tiles": -(-m // TM), "tile_spans_images": c.n > 1 and (ho * wo) % TM != 0, "K": k,
            "steps": -(-k // KE[prec]), "k_tail": k_tail(c, prec), "taps_per_step": max(1, KE[prec] // c.cin)}


def _add(name, n, h, w, cin, cout, k, s, p, cin_w=None, act=ACT_RELU, sliced=True):
    c = ConvCase(name, n, h, w, cin, cin_w or cin, cout, k, s, p, act, 8 if sliced else 0, cin + (24 if sliced else 0),
                 8 if sliced else 0, cout + (16 if sliced else 0), 1000 + len(CONV_CASES))
    assert h != w or h == 1, name
    CONV_CASES[name] = c
    assert c.k[0] * c.k[1] * c.cin <= 4032                       # the exactness argument of the module docstring
    for prec in ("fp32", "bf16"):
        want = expected(name, prec)
        for v in variants(c, prec):
            wrong = _store(_reference(c, v, prec), prec)
            assert not torch.equal(want, wrong), f"{name} [{prec}] cannot tell the right kernel from the '{v}' one"
    return c


# ---- the stem: Cin 16 with 3 weight channels (4 taps per bf16 step, 2 per fp32 step), stride 2, 108 pixels in one tile over two images ----
c = _add("stem_3x3_s2_cin16w3_co48", 2, 13, 19, 16, 48, (3, 3), 2, (0, 0), cin_w=3)
assert branch(c, "bf16")["taps_per_step"] == 4 and branch(c, "fp32")["taps_per_step"] == 2
assert branch(c, "bf16")["M"] < TM and branch(c, "bf16")["ni"] == 2 and branch(c, "bf16")["masked_couts"] == 16
assert set(variants(c, "bf16")) == set(variants(c, "fp32")) == {"transpose", "kdrop"}

# ---- 3x3 valid, Cin 80 (K = 720: a tap boundary inside a step, a 16-element tail), Cout 192 = three two-block tiles, M = 3 * 128 + 1 ----
c = _add("3x3_s1_p0_cin80_co192", 5, 9, 13, 80, 192, (3, 3), 1, (0, 0))
assert branch(c, "fp32")["M"] == 3 * TM + 1 and branch(c, "fp32")["ni"] == 2 and branch(c, "fp32")["cout_tiles"] == 3
assert set(variants(c, "bf16")) == {"transpose", "kdrop"}

# ---- 3x3 pad 1, Cin 448: K = 4032, the network's longest and a whole number of steps; Cout 96 = one-block tiles, exact; M = 2 * 128 ----
c = _add("3x3_s1_p1_cin448_co96", 2, 8, 16, 448, 96, (3, 3), 1, (1, 1))
assert branch(c, "bf16")["K"] == 4032 and not branch(c, "bf16")["k_tail"] and not branch(c, "fp32")["k_tail"]
assert branch(c, "bf16")["M"] == 2 * TM and branch(c, "bf16")["ni"] == 1 and branch(c, "bf16")["masked_couts"] == 0
assert set(variants(c, "bf16")) == {"transpose", "tall"}

# ---- 1x1 ----
c = _add("1x1_cin64_co96", 3, 7, 9, 64, 96, (1, 1), 1, (0, 0))
assert variants(c, "bf16") == [] and branch(c, "bf16")["tile_spans_images"]

# ---- 5x5 pad 2, Cin 48: K = 1200 (tap boundaries inside steps, tails of 48 / 16); Cout 80 = one-block tiles, the last half masked;
#      six 35-pixel maps: every 128-pixel tile spans four images ----
c = _add("5x5_p2_cin48_co80", 6, 5, 7, 48, 80, (5, 5), 1, (2, 2))
assert branch(c, "bf16")["k_tail"] == 48 and branch(c, "fp32")["k_tail"] == 16
assert branch(c, "bf16")["ni"] == 1 and branch(c, "bf16")["masked_couts"] == 16 and c.h * c.w <= 40 and c.n >= 5
assert set(variants(c, "fp32")) == {"transpose", "tall", "kdrop"}

# ---- 1x7 / 7x1, Cin 160, on 36-pixel maps of five images, H < W and H > W ----
for tag, (h, w) in (("wide", (4, 9)), ("tall", (9, 4))):
    c = _add(f"1x7_cin160_co48_{tag}", 5, h, w, 160, 48, (1, 7), 1, (0, 3))
    assert set(variants(c, "bf16")) == {"pads_swapped", "long_row", "kdrop"} and set(variants(c, "fp32")) == {"pads_swapped", "long_row"}
    assert branch(c, "bf16")["tile_spans_images"] and c.h * c.w <= 40
    c = _add(f"7x1_cin160_co192_{tag}", 5, h, w, 160, 192, (7, 1), 1, (3, 0))
    assert set(variants(c, "bf16")) == {"pads_swapped", "tall", "kdrop"} and branch(c, "bf16")["tile_spans_images"]

# ---- 1x3 / 3x1 (Mixed_7*), H < W and H > W; the 1x3 pair fills exactly one 128-pixel tile ----
for tag, (h, w) in (("wide", (4, 8)), ("tall", (8, 4))):
    c = _add(f"1x3_cin64_co96_{tag}", 4, h, w, 64, 96, (1, 3), 1, (0, 1))
    assert set(variants(c, "bf16")) == {"pads_swapped", "long_row"} and branch(c, "bf16")["M"] == TM
for tag, (h, w) in (("wide", (5, 6)), ("tall", (6, 5))):
    c = _add(f"3x1_cin64_co80_{tag}", 3, h, w, 64, 80, (3, 1), 1, (1, 0))
    assert set(variants(c, "bf16")) == {"pads_swapped", "tall"}

# ---- the fc head: 1x1 over N x 1 x 1 pixels, no activation, dense buffers, 1008 of 1024 couts stored ----
c = _add("fc_cin2048_co1008", 3, 1, 1, 2048, 1008, (1, 1), 1, (0, 0), act=ACT_NONE, sliced=False)
assert branch(c, "fp32")["ni"] == 2 and branch(c, "fp32")["cout_tiles"] == 16 and branch(c, "fp32")["masked_couts"] == 16
assert (expected("fc_cin2048_co1008", "fp32") < 0).any()          # ACT_NONE shows: a ReLU would have cleared these

# ---- the > 1 GiB batch split: 16 MiB per image in a 2048-channel fp32 buffer, so 64 images per launch and a second launch of one ----
SPLIT = ConvCase("split_3x3_s1_p1_cin16_co32_n65", 65, 32, 64, 16, 16, 32, (3, 3), 1, (1, 1), ACT_RELU, 1024, 2048, 0, 32, 2000)
assert SPLIT.h * SPLIT.w * SPLIT.ldx * 4 == 1 << 24 and (1 << 30) // (1 << 24) == 64 < SPLIT.n
CONV_CASES[SPLIT.name] = SPLIT                                    # expected(SPLIT.name, "fp32") on demand; not in CONV_NAMES
CONV_NAMES = [n for n in CONV_CASES if n != SPLIT.name]


def first_difference(got, want):
    """'' if equal, else the count of differing elements and the first differing (n, co, oh, ow) with both values."""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = (got.float() != want.float()) | (got.float().isnan())
    if not bad.any():
        return ""
    n, co, oh, ow = (int(v) for v in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first at (n, co, oh, ow) = ({n}, {co}, {oh}, {ow}): "
            f"got {got[n, co, oh, ow].item()}, want {want[n, co, oh, ow].item()}")


# =================================================================================================
# feature statistics
# =================================================================================================
STAT_BATCHES = ([1, 1], [7, 1], [50, 50, 1], [3, 50])
STAT_DIMS = (64, 72, 100, 192)
CONST_COL, TWIN_COLS = 5, (9, 41)


def stat_rows(n, d, seed):
    """(n, d) float32 rows: Gaussian columns (mean 3, deviations 0.1 .. 2), column CONST_COL constant, columns TWIN_COLS equal."""
    rng = np.random.default_rng(seed)
    rows = (3.0 + rng.normal(size=(n, d)) * rng.uniform(0.1, 2.0, d)).astype(np.float32)
    rows[:, CONST_COL] = np.float32(2.7182817)
    rows[:, TWIN_COLS[1]] = rows[:, TWIN_COLS[0]]
    return rows


def float64_stats(rows):
    r = rows.astype(np.float64)
    return r.mean(0), np.cov(r, rowvar=False)


def emulate_stats(batches, shifted=True):
    """wu_feature_stats_update + FIDStatistics.finalize in numpy: shift = fp32 mean of the first batch, x - k in fp32, the shifted column
    sums in fp64 (feature_colsum_kernel), products and per-batch sums of the cross term in fp32 in row order (feature_cross_kernel's MFMA
    chain, up to its summation order), batch totals in fp64, finalize as written.  shifted=False: no shift and every per-batch sum in
    fp32 -- the plain accumulation the shift exists to avoid."""
    d = batches[0].shape[1]
    k = np.zeros(d, np.float32)
    if shifted:
        acc = np.zeros(d, np.float64)
        for row in batches[0]:
            acc += row.astype(np.float64)
        k = (acc / batches[0].shape[0]).astype(np.float32)
    tot_s, tot_c, n = np.zeros(d, np.float64), np.zeros((d, d), np.float64), 0
    for xb in batches:
        xc = xb.astype(np.float32) - k
        sb = np.zeros(d, np.float64 if shifted else np.float32)
        cb = np.zeros((d, d), np.float32)
        for row in xc:
            sb += row.astype(sb.dtype)
            cb += np.outer(row, row)
        tot_s += sb.astype(np.float64)
        tot_c += cb.astype(np.float64)
        n += xb.shape[0]
    m = tot_s / n
    return k.astype(np.float64) + m, (tot_c - n * np.outer(m, m)) / (n - 1)


def stats_error(mu, sigma, want_mu, want_sigma):
    """Worst error of (mu, sigma), each relative to the largest magnitude of its float64 counterpart."""
    return max(np.abs(mu - want_mu).max() / np.abs(want_mu).max(), np.abs(sigma - want_sigma).max() / np.abs(want_sigma).max())


# ---- the stress rows: column means of 1e3 with deviations 0.01 .. 2, batches of 50, 50 and 1 ----
STRESS_BATCHES = (50, 50, 1)
STRESS_D = 72
_rng = np.random.default_rng(77)
STRESS_ROWS = (1e3 + _rng.normal(size=(sum(STRESS_BATCHES), STRESS_D)) * np.geomspace(0.01, 2.0, STRESS_D)).astype(np.float32)


def split_rows(rows, batches):
    edges = np.cumsum([0] + list(batches))
    return [rows[a:b] for a, b in zip(edges[:-1], edges[1:])]


_want = float64_stats(STRESS_ROWS)
STRESS_EMULATION_ERROR = stats_error(*emulate_stats(split_rows(STRESS_ROWS, STRESS_BATCHES)), *_want)
STRESS_BOUND = 4 * STRESS_EMULATION_ERROR          # the MFMA's summation order differs from numpy's: a factor 4 for B <= 50
STRESS_UNSHIFTED_ERROR = stats_error(*emulate_stats(split_rows(STRESS_ROWS, STRESS_BATCHES), shifted=False), *_want)
assert 0 < STRESS_EMULATION_ERROR < 1e-5, STRESS_EMULATION_ERROR
# the case is one the shift is needed for: plain fp32 accumulation of the same rows misses the bound (by orders of magnitude)
assert STRESS_UNSHIFTED_ERROR > 100 * STRESS_BOUND, (STRESS_UNSHIFTED_ERROR, STRESS_BOUND)
