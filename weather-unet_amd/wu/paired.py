"""Paired content preservation: SSIM (Wang et al. 2004), MS-SSIM (Wang et al. 2003), PSNR and MAE of an input batch against its conditioned
outputs -- "is it still the same scene?", the question the set statistics (FID, KID, precision / recall) cannot answer.

    s = ssim(x, fakes)                      # x (B, 3, H, W), fakes (R, B, 3, H, W) as a sweep returns them -> (R, B) float64 CUDA
    m = paired_metrics(x, fakes)            # namedtuple (ssim, ms_ssim, psnr, mae) from one pass
    python -m wu.paired DIR_A DIR_B         # files paired by stem

Semantics, in full (tests/_ssim_ref.py restates them in numpy).  All arithmetic in float64, every operation rounded on its own.  A value is
widened and mapped ``v * scale + shift``: ``value_range=(lo, hi)`` gives ``scale = 1 / (hi - lo)``, ``shift = -lo * scale`` and the data range
``L = 1`` ((-1, 1): ``(v + 1) * 0.5``; (0, 1): identity); ``value_range="uint8"`` is the identity with ``L = 255``.  ``C1 = (K1 L)^2``,
``C2 = (K2 L)^2``.  Window: ``g[t] = exp(-(t - k // 2)^2 / (2 sigma^2))``, ``g /= g.sum()``, k odd in 3..11.  Filter F: valid, along H first and
then along W, taps in ascending order (``a = g[0] v[0]; a = a + g[t] v[t]``); ``x x``, ``y y`` and ``x y`` are formed before filtering.  Over the
(H - k + 1) x (W - k + 1) valid positions

    mxx = mu_x mu_x;  myy = mu_y mu_y;  mxy = mu_x mu_y;      sx = F(x x) - mxx;  sy = F(y y) - myy;  sxy = F(x y) - mxy
    cs   = (2 sxy + C2) / ((sx + sy) + C2)
    ssim = ((2 mxy + C1) / ((mxx + myy) + C1)) cs

``pair_stats`` returns, per (row, image, channel, level), the mean of ``ssim`` and of ``cs``.  SSIM of an image: the mean over channels of the
level-0 ``ssim`` means (``nonnegative=True`` clamps each channel at 0 first).  MS-SSIM: 5 levels, weights (0.0448, 0.2856, 0.3001, 0.2363,
0.1333); between levels both images go through the 2 x 2 mean ``((p00 + p01) + (p10 + p11)) * 0.25`` with ``size % 2`` zero rows / columns in
FRONT of an odd dimension (size s -> s // 2 + s % 2; torch's ``avg_pool2d(padding=[H % 2, W % 2])``); per channel
``prod_l max(v_l, 0)^w_l`` with v_l the ``cs`` mean for l < 4 and the ``ssim`` mean at l = 4, then the mean over channels.
``min(H, W) <= (k - 1) * 16`` raises, it never clamps.  Errors per (row, image): ``sse = sum (x - y)^2`` and ``sae = sum |x - y|`` over all
C H W mapped values, ``mse = sse / (C H W)``, ``psnr = 10 log10(L^2 / mse)`` (inf at 0), ``mae = sae / (C H W)``.

One call of wu_ssim_pairs (csrc/ssim.hip) serves all R rows: x is filtered once per tile, not once per row; inputs go in through their
strides (channels-last, crops, the sweep's (R, B, ...) output, uint8 NHWC as a permuted view) without a copy.  CUDA tensors only: there is
no CPU fallback."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .files import pair_files, paired_batches  # noqa: F401  (pair_files: the name callers know it by here)
from .layout import stream_ptr

U8 = 2                                  # WU_SSIM_U8, next to _lib.F32 / _lib.BF16
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_LEVELS = len(MS_WEIGHTS)
_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: U8}

PairStats = collections.namedtuple("PairStats", "ssim_mean cs_mean err ssim_map numel data_range")
PairedMetrics = collections.namedtuple("PairedMetrics", "ssim ms_ssim psnr mae")


def gaussian_window(size=11, sigma=1.5):
    """The normalised 1-D Gaussian as a float64 numpy array."""
    if int(size) != size or size < 3 or size > 11 or size % 2 == 0:
        raise ValueError(f"gaussian_window: size {size} must be odd and in 3..11")
    t = np.arange(int(size), dtype=np.float64)
    g = np.exp(-(t - int(size) // 2) ** 2 / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def range_mapping(value_range):
    """(scale, shift, L) of a value range: "uint8" or (lo, hi)."""
    if isinstance(value_range, str):
        if value_range != "uint8":
            raise ValueError(f"value_range {value_range!r}: \"uint8\" or a (lo, hi) pair")
        return 1.0, 0.0, 255.0
    lo, hi = (float(v) for v in value_range)
    if not hi > lo:
        raise ValueError(f"value_range {value_range}: hi must exceed lo")
    scale = 1.0 / (hi - lo)
    return scale, -lo * scale, 1.0


def check_ms_size(h, w, win_size, levels):
    if levels > 1 and min(h, w) <= (win_size - 1) * 2 ** (levels - 1):
        raise ValueError(f"MS-SSIM over {levels} levels with a window of {win_size} needs min(H, W) > {(win_size - 1) * 2 ** (levels - 1)}, "
                         f"got {h} x {w}; use a smaller window or ms=False (the size is never clamped silently)")


def pair_stats(x, y, value_range=(-1, 1), win_size=11, sigma=1.5, K=(0.01, 0.03), levels=1, return_map=False):
    """The thin wrapper over wu_ssim_pairs.  x (B, C, H, W); y (B, C, H, W) or (R, B, C, H, W); float32, bfloat16 or uint8 CUDA tensors of
    any strides (two floating dtypes that differ are both taken as float32).  Returns PairStats of float64 CUDA tensors, with the leading R
    only when y has it: ssim_mean / cs_mean (R, B, C, levels), err (R, B, 2) = (sse, sae), ssim_map (R, B, C, H - k + 1, W - k + 1) or None;
    numel = C H W and data_range = L go with them.  Nothing is synchronised."""
    if not (torch.is_tensor(x) and torch.is_tensor(y) and x.is_cuda and y.is_cuda):
        raise RuntimeError("wu.paired: CUDA tensors only -- no CPU fallback")
    if x.dim() != 4 or y.dim() not in (4, 5) or tuple(y.shape[-4:]) != tuple(x.shape) or x.device != y.device:
        raise ValueError(f"pair_stats: x (B, C, H, W) and y (B, C, H, W) or (R, B, C, H, W) on one device, got {tuple(x.shape)} / {tuple(y.shape)}")
    if levels not in (1, MS_LEVELS):
        raise ValueError(f"pair_stats: levels {levels} must be 1 or {MS_LEVELS}")
    window = gaussian_window(win_size, sigma)
    k = len(window)
    b, c, h, w = x.shape
    if h < k or w < k:
        raise ValueError(f"pair_stats: image {h} x {w} is smaller than the window {k}")
    check_ms_size(h, w, k, levels)
    x, y = x.detach(), y.detach()
    if x.dtype != y.dtype and x.is_floating_point() and y.is_floating_point():
        x, y = x.float(), y.float()
    if x.dtype != y.dtype or x.dtype not in _DTYPES:
        raise ValueError(f"pair_stats: float32, bfloat16 or uint8 on both sides, got {x.dtype} / {y.dtype}")
    scale, shift, data_range = range_mapping(value_range)
    squeeze = y.dim() == 4
    y5 = y.unsqueeze(0) if squeeze else y
    r = y5.shape[0]
    lib = _lib.load()
    dev = x.device
    nbytes = lib.wu_ssim_workspace_bytes(b, r, c, h, w, k, levels)
    if nbytes == 0:
        raise ValueError(f"pair_stats: B {b} R {r} C {c} H {h} W {w} out of the kernel's range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ssim_mean = torch.empty(r, b, c, levels, dtype=torch.float64, device=dev)
    cs_mean = torch.empty_like(ssim_mean)
    err = torch.empty(r, b, 2, dtype=torch.float64, device=dev)
    smap = torch.empty(r, b, c, h - k + 1, w - k + 1, dtype=torch.float64, device=dev) if return_map else None
    win = (ctypes.c_double * k)(*window.tolist())
    with torch.cuda.device(dev):
        _lib.call("wu_ssim_pairs", x.data_ptr(), *x.stride(), y5.data_ptr(), *y5.stride(), _DTYPES[x.dtype], b, r, c, h, w, scale, shift,
                  data_range, float(K[0]), float(K[1]), win, k, levels, ws.data_ptr(), ssim_mean.data_ptr(), cs_mean.data_ptr(),
                  err.data_ptr(), smap.data_ptr() if return_map else None, stream_ptr())
    out = (ssim_mean, cs_mean, err, smap)
    if squeeze:
        out = tuple(t[0] if t is not None else None for t in out)
    return PairStats(*out, c * h * w, data_range)


def combine_ssim(stats, nonnegative=False):
    """SSIM per image from PairStats: the mean over channels of the level-0 ssim means."""
    v = stats.ssim_mean[..., 0]
    if nonnegative:
        v = v.clamp(min=0)
    return v.mean(-1)


def combine_ms_ssim(stats, weights=MS_WEIGHTS):
    """MS-SSIM per image from PairStats of len(weights) levels: prod_l max(v_l, 0)^w_l per channel, then the mean over channels."""
    n = stats.ssim_mean.shape[-1]
    if n != len(weights) or n < 2:
        raise ValueError(f"combine_ms_ssim: {len(weights)} weights for statistics of {n} levels")
    v = torch.cat([stats.cs_mean[..., :n - 1], stats.ssim_mean[..., n - 1:]], -1).clamp(min=0)
    w = torch.tensor(weights, dtype=torch.float64, device=v.device)
    return (v ** w).prod(-1).mean(-1)


def mse_of(stats):
    return stats.err[..., 0] / stats.numel


def mae_of(stats):
    return stats.err[..., 1] / stats.numel


def psnr_of(stats):
    return 10.0 * torch.log10(stats.data_range * stats.data_range / mse_of(stats))


def ssim(x, y, value_range=(-1, 1), win_size=11, sigma=1.5, K=(0.01, 0.03), nonnegative=False):
    """SSIM of every pair: (R, B) or (B,) float64 CUDA."""
    return combine_ssim(pair_stats(x, y, value_range, win_size, sigma, K), nonnegative)


def ms_ssim(x, y, value_range=(-1, 1), win_size=11, sigma=1.5, K=(0.01, 0.03), weights=MS_WEIGHTS):
    """MS-SSIM of every pair over five levels: (R, B) or (B,) float64 CUDA.  ValueError when min(H, W) <= (win_size - 1) * 16."""
    return combine_ms_ssim(pair_stats(x, y, value_range, win_size, sigma, K, MS_LEVELS), weights)


def psnr(x, y, value_range=(-1, 1)):
    """PSNR of every pair in dB (inf for identical images): (R, B) or (B,) float64 CUDA."""
    win = min(11, (min(x.shape[-2:]) - 1) // 2 * 2 + 1)          # the error sums do not depend on the window: any legal one
    return psnr_of(pair_stats(x, y, value_range, win))


def paired_metrics(x, y, value_range=(-1, 1), win_size=11, sigma=1.5, K=(0.01, 0.03), ms=True):
    """(ssim, ms_ssim, psnr, mae) of every pair from ONE pass; ms_ssim is None with ms=False."""
    st = pair_stats(x, y, value_range, win_size, sigma, K, MS_LEVELS if ms else 1)
    return PairedMetrics(combine_ssim(st), combine_ms_ssim(st) if ms else None, psnr_of(st), mae_of(st))


# ----------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------
def metrics_of_dirs(dir_a, dir_b, ms=True, win_size=11, batch_size=32, device="cuda:0"):
    """The means over the paired files of two directories of the per-pair SSIM, MS-SSIM (None with ms=False), PSNR and MAE (in grey levels):
    {"ssim", "ms_ssim", "psnr", "mae", "pairs"}.  Files are read with Pillow as uint8 RGB; a pair of unequal size is an error; pairs are
    batched by size (``wu.files.paired_batches``)."""
    sums, count = None, 0
    for xa, xb in paired_batches(dir_a, dir_b, batch_size, device):
        m = paired_metrics(xa, xb, "uint8", win_size, ms=ms)
        part = torch.stack([v.sum() for v in m if v is not None])
        sums = part if sums is None else sums + part
        count += xa.shape[0]
    vals = (sums / count).tolist()
    return {"ssim": vals[0], "ms_ssim": vals[1] if ms else None, "psnr": vals[-2], "mae": vals[-1], "pairs": count}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wu.paired", description="SSIM / MS-SSIM / PSNR / MAE of two directories paired by file stem")
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--no-ms", action="store_true", help="skip MS-SSIM (needed for images of min(H, W) <= 16 (win - 1))")
    ap.add_argument("--win", type=int, default=11, help="window size, odd, 3..11")
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args(argv)
    r = metrics_of_dirs(args.dir_a, args.dir_b, not args.no_ms, args.win, args.batch_size)
    print(f"SSIM: {r['ssim']:.6f}")
    if r["ms_ssim"] is not None:
        print(f"MS-SSIM: {r['ms_ssim']:.6f}")
    print(f"PSNR: {r['psnr']:.4f} dB" if math.isfinite(r["psnr"]) else "PSNR: inf dB")
    print(f"MAE: {r['mae']:.6f}")
    print(f"pairs: {r['pairs']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
