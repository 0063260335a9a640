"""Full-resolution output: the network's low-resolution result carried back onto the photograph's own pixel grid by the fast colour guided
filter (He, Sun, Tang 2013; He, Sun 2015).

    up = GuidedUpsampler(r=4, eps=1e-3)
    u8 = up.upsample(batch, low, photos_u8, sizes)      # batch (N, 3, S, S) in [-1, 1] as the input pipeline makes it, low (R, N, 3, S, S)
                                                        # in [0, 1], photos (N, Hmax, Wmax, 3) uint8 with per-image (h, w)
                                                        # -> (R, N, Hmax, Wmax, 3) uint8, what the encoders take with ``sizes``

Two stages (csrc/guided.hip; tests/_guided_ref.py restates the arithmetic in numpy, include/wu_kernels.h states it in full):

* ``coefficients``: at low resolution, per pixel, the local affine model ``q = A I + b`` from the guide ``I`` (the network's input) to each
  target ``p`` (the network's output) over the (2r+1)^2 window clipped to the image -- ``A = (Sigma + eps 1)^-1 cov(I, p)``,
  ``b = mean(p) - A mean(I)`` -- and the window mean of ``A`` and ``b``: twelve float64 maps per target.  The guide's moments and the 3 x 3
  inverse are formed once per image and shared by all R targets.
* ``apply``: per photograph pixel the twelve coefficients are interpolated bilinearly (``align_corners=False`` positions) and applied to the
  photograph's own RGB value / 255.  Edges and texture come from the photograph, the change of appearance from the network.  One kernel reads
  every photograph pixel once and writes bytes (``floor(clamp(q * 255, 0, 255))``, ``infer_driver.to_uint8``'s truncation) or float32; no
  full-resolution coefficient map exists in memory.

The two parameters belong to the method, they are not measurements: ``r`` is the window radius in LOW-resolution pixels (larger: smoother
coefficient fields, less of the network's local detail; ``r >= max(hl, wl)`` is one global colour transform per image), ``eps`` the
regulariser added to the guide's covariance in [0, 1]^2 units (larger: ``A`` shrinks towards 0 and the output towards the blurred target;
smaller: the model follows the guide's edges more closely and amplifies noise in flat regions).  The defaults r = 4, eps = 1e-3 are a
starting point and have NOT been tuned on this model's outputs.

All arithmetic is float64 with every operation rounded on its own and no atomics: two runs give the same bits, and an (R, N) call equals R
(N) calls.  CUDA tensors only: there is no CPU fallback."""
import ctypes

import torch

from . import _lib
from .layout import stream_ptr
from .paired import range_mapping

_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def _require_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"GuidedUpsampler: {what} must be a CUDA tensor -- no CPU fallback")


class GuidedUpsampler:
    """See the module docstring.  Owns a grow-only workspace; nothing is synchronised."""

    def __init__(self, r=4, eps=1e-3):
        if int(r) != r or r < 0:
            raise ValueError(f"GuidedUpsampler: radius r {r} must be a non-negative integer")
        if not eps > 0:
            raise ValueError(f"GuidedUpsampler: eps {eps} must be positive")
        self.r, self.eps = int(r), float(eps)
        self._ws = None

    def _workspace(self, nbytes, dev):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    def coefficients(self, guide_lo, targets_lo, guide_range=(-1, 1), target_range=(0, 1)):
        """guide_lo (N, 3, hl, wl) float; targets_lo (N, 3, hl, wl) or (R, N, 3, hl, wl), float32 or bfloat16; any strides (the sweep's
        output goes in without a copy).  Returns the float64 coefficient maps (R, N, 12, hl, wl) -- without the leading R when the targets
        have none: mean(a_ck) at map 3 c + k, mean(b_c) at map 9 + c."""
        _require_cuda(guide_lo, "guide_lo")
        _require_cuda(targets_lo, "targets_lo")
        if guide_lo.dim() != 4 or guide_lo.shape[1] != 3 or targets_lo.dim() not in (4, 5) or tuple(targets_lo.shape[-4:]) != tuple(guide_lo.shape) \
                or guide_lo.device != targets_lo.device:
            raise ValueError(f"GuidedUpsampler.coefficients: guide (N, 3, hl, wl) and targets (N, 3, hl, wl) or (R, N, 3, hl, wl) on one device, "
                             f"got {tuple(guide_lo.shape)} / {tuple(targets_lo.shape)}")
        guide, targets = guide_lo.detach(), targets_lo.detach()
        if guide.dtype != torch.float32:
            guide = guide.float()
        if targets.dtype not in _DTYPES:
            targets = targets.float()
        squeeze = targets.dim() == 4
        t5 = targets.unsqueeze(0) if squeeze else targets
        rr, n, _, hl, wl = t5.shape
        if min(rr, n, hl, wl) < 1:
            raise ValueError(f"GuidedUpsampler.coefficients: empty input {tuple(targets_lo.shape)}")
        gsc, gsh = range_mapping(guide_range)[:2]              # (lo, hi) -> (0, 1): scale = 1 / (hi - lo), shift = -lo * scale
        tsc, tsh = range_mapping(target_range)[:2]
        lib, dev = _lib.load(), guide.device
        nbytes = lib.wu_guided_workspace_bytes(n, rr, hl, wl)
        if nbytes == 0:
            raise ValueError(f"GuidedUpsampler.coefficients: N {n} R {rr} hl {hl} wl {wl} out of the kernel's range")
        ws = self._workspace(nbytes, dev)
        out = torch.empty(rr, n, 12, hl, wl, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.call("wu_guided_coeffs", guide.data_ptr(), *guide.stride(), gsc, gsh, t5.data_ptr(), *t5.stride(), _DTYPES[t5.dtype], tsc, tsh,
                      n, rr, hl, wl, self.r, self.eps, ws.data_ptr(), out.data_ptr(), stream_ptr())
        return out[0] if squeeze else out

    def apply(self, coeffs, photos_u8, sizes, out="uint8"):
        """coeffs (R, N, 12, hl, wl) or (N, 12, hl, wl) float64 from ``coefficients``; photos_u8 (N, Hmax, Wmax, 3) uint8 as the decoders
        leave them, ``sizes`` N x (h, w).  Returns, with the leading R only when the coefficients have it, ``out="uint8"``: the padded
        (R, N, Hmax, Wmax, 3) bytes the encoders take with ``sizes``; ``out="float"``: (R, N, 3, Hmax, Wmax) float32.  What lies outside an
        image's (h, w) is not written (uninitialised memory of a fresh tensor)."""
        _require_cuda(coeffs, "coeffs")
        _require_cuda(photos_u8, "photos_u8")
        if out not in ("uint8", "float"):
            raise ValueError(f"GuidedUpsampler.apply: out {out!r} must be \"uint8\" or \"float\"")
        if coeffs.dtype != torch.float64 or coeffs.dim() not in (4, 5) or coeffs.shape[-3] != 12:
            raise ValueError(f"GuidedUpsampler.apply: float64 coefficients (R, N, 12, hl, wl) or (N, 12, hl, wl), got {tuple(coeffs.shape)} {coeffs.dtype}")
        if photos_u8.dtype != torch.uint8 or photos_u8.dim() != 4 or photos_u8.shape[3] != 3 or not photos_u8.is_contiguous():
            raise ValueError("GuidedUpsampler.apply: expected a contiguous (N, Hmax, Wmax, 3) uint8 tensor")
        squeeze = coeffs.dim() == 4
        c5 = (coeffs.unsqueeze(0) if squeeze else coeffs).contiguous()
        rr, n, _, hl, wl = c5.shape
        nn, hmax, wmax, _ = photos_u8.shape
        if nn != n or coeffs.device != photos_u8.device:
            raise ValueError(f"GuidedUpsampler.apply: coefficients of {n} images for {nn} photographs (on one device)")
        sizes = [(int(h), int(w)) for h, w in sizes]
        if len(sizes) != n or any(h < 1 or w < 1 or h > hmax or w > wmax for h, w in sizes):
            raise ValueError("GuidedUpsampler.apply: sizes must give one (h, w) <= (Hmax, Wmax) per image")
        dev = coeffs.device
        flat = [v for hw in sizes for v in hw]
        host = (ctypes.c_int * (2 * n))(*flat)
        sizes_d = torch.tensor(flat, dtype=torch.int32).to(dev)
        if out == "uint8":
            res = torch.empty(rr, n, hmax, wmax, 3, dtype=torch.uint8, device=dev)
            u8p, f32p = res.data_ptr(), None
        else:
            res = torch.empty(rr, n, 3, hmax, wmax, dtype=torch.float32, device=dev)
            u8p, f32p = None, res.data_ptr()
        with torch.cuda.device(dev):
            _lib.call("wu_guided_apply", c5.data_ptr(), n, rr, hl, wl, photos_u8.data_ptr(), hmax, wmax, host, sizes_d.data_ptr(), u8p, f32p,
                      stream_ptr())
        return res[0] if squeeze else res

    def upsample(self, guide_lo, targets_lo, photos_u8, sizes, guide_range=(-1, 1), target_range=(0, 1), out="uint8"):
        """``apply(coefficients(guide_lo, targets_lo, ...), photos_u8, sizes, out)``."""
        return self.apply(self.coefficients(guide_lo, targets_lo, guide_range, target_range), photos_u8, sizes, out)
