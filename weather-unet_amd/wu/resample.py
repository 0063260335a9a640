"""Pillow-exact antialiased resampling on the GPU, in front of the metrics (csrc/resample.hip; C ABI: include/wu_kernels.h).

``GPUResampler(size, filter, mode)`` resizes a batch to one ``size`` with Pillow's box, bilinear, bicubic or Lanczos filter:

* ``mode="u8"`` equals ``Image.resize`` on RGB uint8 images bit for bit (fixed-point coefficients, 8-bit intermediate);
* ``mode="f32"`` equals ``Image.resize`` on each channel as a mode ``'F'`` image: float64 sums, a float32 intermediate, no quantisation
  and no clipping inside the resize (bicubic and Lanczos overshoot [0, 255]).  This is the "clean" resize of Parmar et al. (CVPR 2022).

The batch is the padded ragged uint8 batch ``(N, Hmax, Wmax, 3)`` plus per-image ``(h, w)`` that ``wu.jpeg.GPUJpegDecoder.decode_batch``,
``wu.png.GPUPngDecoder`` and ``wu.png.decode_mixed`` return -- one launch serves images of different sizes -- or an fp32 / bf16
``(N, 3, H, W)`` tensor of one size, read through its strides (channels-last and cropped views are fine).

The coefficient tables are Resample.c's ``precompute_coeffs`` in float64, built here on the host and cached by (in, out, filter): the three
arithmetic filters with numpy (every operation one IEEE operation, the normalising sum accumulated in tap order), Lanczos with
``math.sin``, the C library's, which is what Pillow calls (``numpy.sin`` and the device's ``sin`` differ from it in the last bit).
There is no host fallback for the resize itself."""
import math

import numpy as np
import torch

from . import _lib
from .files import padded_batch, read_batches, resize_files  # noqa: F401  (they read files for this module: wu.files)
from .layout import empty_nhwc, require_cuda, stream_ptr, torch_dtype

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 22
MAX_OUT = 1024
_OUT = {"nhwc_u8": 0, "raw": 1, "unit": 2, "nchw": 3, "inception": 4}
_MODE_U8, _NORMALIZE, _RANGE_PM1 = 1, 1 << 16, 1 << 17
_DESC = np.dtype([("src_off", "<i8"), ("s_row", "<i8"), ("s_col", "<i8"), ("s_ch", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"),
                  ("hb", "<i4"), ("hk", "<i4"), ("vb", "<i4"), ("vk", "<i4"), ("kx", "<i4"), ("ky", "<i4")])


def _filter_values(name, x):
    """The filter at every entry of the float64 array ``x`` (Resample.c's *_filter functions, operation by operation)."""
    if name == "box":
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    if name == "bilinear":
        a = np.abs(x)
        return np.where(a < 1.0, 1.0 - a, 0.0)
    if name == "bicubic":                                           # a = -0.5
        a = np.abs(x)
        near = ((1.5 * a - 2.5) * a) * a + 1
        far = (((a - 5) * a + 8) * a - 4) * -0.5
        return np.where(a < 1.0, near, np.where(a < 2.0, far, 0.0))
    if name == "lanczos":
        def sinc(v):
            if v == 0.0:
                return 1.0
            v = v * math.pi
            return math.sin(v) / v
        flat = [sinc(v) * sinc(v / 3) if -3.0 <= v < 3.0 else 0.0 for v in x.ravel().tolist()]
        return np.array(flat, dtype=np.float64).reshape(x.shape)
    raise ValueError(f"filter must be one of {FILTERS}, got {name!r}")


def coefficients(in_size, out_size, filter):
    """Resample.c precompute_coeffs for one axis: (bounds (out, 2) int32 = [first source index, count], kk (out, ksize) float64,
    normalised; entries at and beyond ``count`` are 0)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filter] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)             # C's (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < xmax[:, None]
    w = np.where(live, _filter_values(filter, ((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for k in range(ksize):                                                       # the sum in tap order
        ww = ww + w[:, k]
    w = np.where(live & (ww[:, None] != 0.0), w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    return np.stack([xmin, xmax], axis=1).astype(np.int32), w


def coefficients_8bpc(kk):
    """Resample.c normalize_coeffs_8bpc: (int)(+-0.5 + w * 2^22), truncated toward zero."""
    v = kk * float(1 << PRECISION_BITS)
    return np.where(kk < 0, -0.5 + v, 0.5 + v).astype(np.int64).astype(np.int32)


def _pair(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


class GPUResampler:
    """``GPUResampler(size, filter="bicubic", mode="f32" | "u8", out=..., band=None)(batch, sizes=None, value_range=(0, 1))``.

    ``size``: an int or (H, W), at most 1024 a side.  ``out``:
      "nchw"     (N, 3, H, W) float32, ``clip(v, 0, 255) / 255`` then ``(x - 0.5) / 0.5`` (ToTensor + Normalize(0.5, 0.5));
      "unit"     (N, 3, H, W) float32, ``clip(v, 0, 255) / 255``;
      "raw"      (N, 3, H, W) float32, Pillow's value itself: 0..255, unclipped in float mode;
      "nhwc_u8"  (N, H, W, 3) uint8 (``mode="u8"`` only), the batch the JPEG / PNG encoders and wu.grid take.
    ``band``: output rows per workgroup (1..8; None: the kernel's default); every value gives the same bits.
    ``batch``: (N, Hmax, Wmax, 3) uint8 with ``sizes`` = [(h, w)] per image (None: every image fills the batch), or (N, 3, H, W) float32 /
    bfloat16 with values in ``value_range`` (0, 1) or (-1, 1); in 8-bit mode a float source is quantised first as
    ``wu.infer_driver.to_uint8`` does.  Runs on the current torch stream."""

    def __init__(self, size, filter="bicubic", mode="f32", out="nchw", band=None):
        self.size = _pair(size)
        if min(self.size) < 1 or max(self.size) > MAX_OUT:
            raise ValueError(f"GPUResampler: the output side must be 1..{MAX_OUT} (one thread per output column), got {self.size}")
        if filter not in FILTERS:
            raise ValueError(f"GPUResampler: filter must be one of {FILTERS}, got {filter!r}")
        if mode not in ("f32", "u8"):
            raise ValueError(f"GPUResampler: mode must be 'f32' or 'u8', got {mode!r}")
        if out not in ("nchw", "unit", "raw", "nhwc_u8"):
            raise ValueError(f"GPUResampler: out must be 'nchw', 'unit', 'raw' or 'nhwc_u8', got {out!r}")
        if out == "nhwc_u8" and mode != "u8":
            raise ValueError("GPUResampler: out='nhwc_u8' needs mode='u8' (the float mode does not quantise)")
        max_band = _lib.load().wu_resample_max_band()
        if band is not None and not 1 <= int(band) <= max_band:
            raise ValueError(f"GPUResampler: band must be 1..{max_band}, got {band}")
        self.filter, self.mode, self.out, self.band = filter, mode, out, 0 if band is None else int(band)
        self._tables = {}                     # (in, out) -> (bounds, coefficients as the kernel reads them, ksize); filter and mode are the object's
        self._ws = None
        self.workspace_growths = 0

    # ---- tables ----
    def _table(self, in_size, out_size, tap_major):
        key = (in_size, out_size, tap_major)
        t = self._tables.get(key)
        if t is None:
            bounds, kk = coefficients(in_size, out_size, self.filter)
            if self.mode == "u8":
                kk = coefficients_8bpc(kk)
            if tap_major:
                kk = kk.T
            t = (np.ascontiguousarray(bounds).tobytes(), np.ascontiguousarray(kk).tobytes(), kk.shape[0] if tap_major else kk.shape[1])
            self._tables[key] = t
        return t

    # ---- the launch ----
    def _source(self, batch, sizes, value_range):
        if batch.dtype == torch.uint8:
            if batch.dim() != 4 or batch.shape[3] != 3:
                raise ValueError(f"GPUResampler: a uint8 batch must be (N, Hmax, Wmax, 3), got {tuple(batch.shape)}")
            n, hm, wm, _ = batch.shape
            sn, sh, sw, sc = batch.stride()
            if sizes is None:
                sizes = [(hm, wm)] * n
            kind, rng = 0, 0
        elif batch.dtype in (torch.float32, torch.bfloat16):
            if batch.dim() != 4 or batch.shape[1] != 3:
                raise ValueError(f"GPUResampler: a float batch must be (N, 3, H, W), got {tuple(batch.shape)}")
            if sizes is not None:
                raise ValueError("GPUResampler: sizes go with the padded uint8 batch; a float batch has one size")
            n, _, hm, wm = batch.shape
            sn, sc, sh, sw = batch.stride()
            sizes = [(hm, wm)] * n
            if tuple(value_range) == (0, 1):
                rng = 0
            elif tuple(value_range) == (-1, 1):
                rng = _RANGE_PM1
            else:
                raise ValueError(f"value_range must be (0, 1) or (-1, 1), got {value_range}")
            kind = 1 if batch.dtype == torch.float32 else 2
        else:
            raise TypeError(f"GPUResampler: the batch must be uint8 NHWC or float32 / bfloat16 NCHW, got {batch.dtype}")
        sizes = [(int(h), int(w)) for h, w in sizes]
        if len(sizes) != n or n == 0:
            raise ValueError(f"GPUResampler: {len(sizes)} sizes for a batch of {n}")
        for h, w in sizes:
            if not (1 <= h <= hm and 1 <= w <= wm):
                raise ValueError(f"GPUResampler: an image of {h} x {w} in a batch padded to {hm} x {wm}")
        return kind, rng, n, sizes, (sn, sh, sw, sc)

    def plan(self, sizes, strides):
        """What the kernel reads besides the pixels, built on the host: (the N descriptors, the workspace image = descriptors + the tables
        of this batch, each distinct table once).  ``strides``: element strides (image, row, column, channel) of the source."""
        n = len(sizes)
        sn, sh, sw, sc = strides
        ho, wo = self.size
        desc = np.zeros(n, dtype=_DESC)
        parts, where, off = [], {}, n * _DESC.itemsize

        def place(blob):
            nonlocal off
            at = where.get(id(blob))
            if at is None:
                at = where[id(blob)] = off
                parts.append(blob)
                off += (len(blob) + 7) & ~7
                if len(blob) & 7:
                    parts.append(b"\0" * (8 - (len(blob) & 7)))
            return at

        for i, (h, w) in enumerate(sizes):
            d = desc[i]
            d["src_off"], d["s_row"], d["s_col"], d["s_ch"], d["src_h"], d["src_w"] = i * sn, sh, sw, sc, h, w
            if w != wo:
                b, k, d["kx"] = self._table(w, wo, True)
                d["hb"], d["hk"] = place(b), place(k)
            if h != ho:
                b, k, d["ky"] = self._table(h, ho, False)
                d["vb"], d["vk"] = place(b), place(k)
        if off >= 1 << 31:
            raise ValueError("GPUResampler: the coefficient tables of this batch exceed 2 GiB")
        return desc, desc.tobytes() + b"".join(parts)

    def _launch(self, batch, sizes, value_range, epi, dst, ldy=0, cpad=0, code=0, normalize=False):
        require_cuda(batch, "GPUResampler")
        kind, rng, n, sizes, strides = self._source(batch, sizes, value_range)
        ho, wo = self.size
        if n * ho * wo >= 1 << 31:
            raise ValueError(f"GPUResampler: N * Hout * Wout must stay below 2^31, got {n} x {ho} x {wo}")
        lib = _lib.load()
        assert lib.wu_resample_desc_bytes() == _DESC.itemsize
        desc, image = self.plan(sizes, strides)
        nbytes = lib.wu_resample_workspace_bytes(n, len(image) - n * _DESC.itemsize)
        dev = batch.device
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=dev)
            self.workspace_growths += 1
        self._ws[:len(image)].copy_(torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()))
        flags = (_MODE_U8 if self.mode == "u8" else 0) | (epi << 4) | (self.band << 8) | (_NORMALIZE if normalize else 0) | rng
        _lib.call("wu_resample", batch.data_ptr(), kind, desc.ctypes.data, self._ws.data_ptr(), self._ws.numel(), n, ho, wo,
                  dst.data_ptr(), ldy, cpad, code, flags, stream_ptr())
        return dst

    def __call__(self, batch, sizes=None, value_range=(0, 1)):
        n = batch.shape[0]
        ho, wo = self.size
        if self.out == "nhwc_u8":
            dst = torch.empty((n, ho, wo, 3), dtype=torch.uint8, device=batch.device)
        else:
            dst = torch.empty((n, 3, ho, wo), dtype=torch.float32, device=batch.device)
        return self._launch(batch, sizes, value_range, _OUT[self.out], dst)

    def inception_input(self, batch, sizes=None, value_range=(0, 1), cpad=16, code=_lib.F32, normalize=True):
        """The InceptionV3 network input itself: (N, cpad, H, W) NHWC storage of dtype ``code``, ``x = clip(v, 0, 255) / 255`` and then the
        ``2x - 1`` and the dtype conversion ``wu_inception_input`` applies to a (0, 1) float image of the network's size."""
        ho, wo = self.size
        x = empty_nhwc(batch.shape[0], cpad, ho, wo, torch_dtype(code), batch.device)
        self._launch(batch, sizes, value_range, _OUT["inception"], x, cpad, cpad, code, normalize)
        return x
