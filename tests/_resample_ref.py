"""Restatement of Pillow's ImagingResample (libImaging/Resample.c) for the box, bilinear, bicubic and Lanczos filters, in its 8-bit form
(Image.resize on RGB uint8) and its float form (Image.resize on a mode 'F' image, per channel).  Scalar Python for the coefficients
(every operation one float64 operation, in Resample.c's order; ``math.sin`` is the C library's); numpy over rows and channels for the two
passes, one tap at a time so that sums run in ascending source order.  tests/test_resample_cpu.py holds it to Pillow bit for bit; the
GPU tests use it where Pillow has no such input (float sources)."""
import math

import numpy as np

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 32 - 8 - 2


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


_FILTER = {"box": _box, "bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def precompute_coeffs(in_size, out_size, name):
    """[(xmin, [w0, w1, ...])] per output coordinate: len(w) = xmax, normalised float64 weights."""
    f = _FILTER[name]
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = SUPPORT[name] * filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            w = f((x + xmin - center + 0.5) * ss)
            ws.append(w)
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        out.append((xmin, ws))
    return out


def _fixed(w):
    return int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))


def _clip8(v):
    return np.clip(v >> PRECISION_BITS, 0, 255)


def _pass_u8(img, coeffs, axis):
    """One pass over ``axis`` of an (h, w, 3) uint8 image: int32 sums from 2^21, clip8."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(coeffs),) + src.shape[1:], dtype=np.uint8)
    for xx, (xmin, ws) in enumerate(coeffs):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for k, w in enumerate(ws):
            acc = acc + src[xmin + k] * _fixed(w)
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)              # int32 arithmetic (never wraps for normalised weights)
        out[xx] = _clip8(acc)
    return np.moveaxis(out, 0, axis)


def _pass_f32(img, coeffs, axis):
    """One pass over ``axis`` of an (h, w, 3) float32 image: float64 sums from 0 in ascending source order, one rounding to float32."""
    src = np.moveaxis(img, axis, 0).astype(np.float64)
    out = np.empty((len(coeffs),) + src.shape[1:], dtype=np.float32)
    for xx, (xmin, ws) in enumerate(coeffs):
        acc = np.zeros(src.shape[1:], dtype=np.float64)
        for k, w in enumerate(ws):
            acc = acc + src[xmin + k] * w
        out[xx] = acc.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def resize(img, size, name, mode):
    """``img`` (h, w, 3): uint8 (mode "u8") or float32 on the 0..255 scale (mode "f32") -> (oh, ow, 3) of the same dtype.  Horizontal pass
    first; a pass between equal sizes is skipped."""
    oh, ow = size
    h, w = img.shape[:2]
    one = _pass_u8 if mode == "u8" else _pass_f32
    assert img.dtype == (np.uint8 if mode == "u8" else np.float32)
    if w != ow:
        img = one(img, precompute_coeffs(w, ow, name), 1)
    if h != oh:
        img = one(img, precompute_coeffs(h, oh, name), 0)
    return np.ascontiguousarray(img)


def to_scale_255(x, value_range):
    """A float32 array in ``value_range`` on the 0..255 scale, in float32 with one rounding per operation."""
    x = x.astype(np.float32)
    if tuple(value_range) == (0, 1):
        return x * np.float32(255.0)
    return x * np.float32(127.5) + np.float32(127.5)


def quantise(t):
    """wu.infer_driver.to_uint8 on the 0..255 scale: clamp, truncate."""
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


# ---- the epilogues of wu.resample.GPUResampler, on Pillow's (or resize()'s) value ----
def unit(v):
    return np.clip(v.astype(np.float32), np.float32(0), np.float32(255)) / np.float32(255.0)


def normalised(v):
    return (unit(v) - np.float32(0.5)) / np.float32(0.5)
