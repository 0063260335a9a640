"""numpy float64 restatement of csrc/guided.hip (include/wu_kernels.h states the same arithmetic): the fast colour guided filter as a joint
upsampler.  Every operation is one IEEE float64 operation in the order written here; sums are written out tap by tap (no ``.sum()``), so
the GPU kernels can be compared with ``np.array_equal``."""
import numpy as np


def map_values(v, scale, shift):
    """A stored value widened to float64, then v * scale + shift in two roundings."""
    v = np.asarray(v).astype(np.float64) * np.float64(scale)
    return v + np.float64(shift)


def range_mapping(value_range):
    """(scale, shift) that carries (lo, hi) to (0, 1): (-1, 1) -> (0.5, 0.5), (0, 1) -> (1, 0)."""
    lo, hi = (float(v) for v in value_range)
    scale = 1.0 / (hi - lo)
    return scale, -lo * scale


def window_counts(n, r):
    """Per position of an axis of n samples: how many of the taps i - r .. i + r lie inside it."""
    i = np.arange(n)
    return np.minimum(n - 1, i + r) - np.maximum(0, i - r) + 1


def _running(v, r, axis):
    """Per position along `axis` the in-range taps i - r .. i + r added in ascending order: s = v[i0]; s = s + v[i0 + 1]; ..."""
    v = np.moveaxis(v, axis, -1)
    n = v.shape[-1]
    r = min(int(r), n)                                       # beyond the axis the window is the whole axis: the same taps
    acc = np.zeros_like(v)
    started = np.zeros(n, dtype=bool)
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(n, n - d)                   # positions i with i + d inside the axis
        if lo >= hi:
            continue
        seg = v[..., lo + d:hi + d]
        first = ~started[lo:hi]
        acc[..., lo:hi] = np.where(first, seg, acc[..., lo:hi] + seg)
        started[lo:hi] = True
    return np.moveaxis(acc, -1, axis)


def box(v, r):
    """The mean over the (2r+1)^2 window clipped to the image, over the last two axes: row sums left to right, the rows of row sums top to
    bottom, one division by count_y * count_x."""
    h, w = v.shape[-2:]
    s = _running(_running(v, r, -1), r, -2)
    cnt = (window_counts(h, r)[:, None] * window_counts(w, r)[None, :]).astype(np.float64)
    return s / cnt


def coefficients(guide, targets, r, eps, guide_scale_shift=(0.5, 0.5), target_scale_shift=(1.0, 0.0)):
    """guide (N, 3, hl, wl), targets (R, N, 3, hl, wl), stored values (float32, or bfloat16 values held in float32) -> (R, N, 12, hl, wl)
    float64: box(a_ck) at map 3 c + k, box(b_c) at map 9 + c.  Asserts det > 0 everywhere."""
    I = map_values(guide, *guide_scale_shift)
    p = map_values(targets, *target_scale_shift)
    assert I.ndim == 4 and p.ndim == 5 and I.shape[1] == 3 and p.shape[1:] == I.shape and r >= 0 and eps > 0
    eps = np.float64(eps)
    mI = [box(I[:, k], r) for k in range(3)]
    S = {}
    for j in range(3):
        for k in range(j, 3):
            S[j, k] = box(I[:, j] * I[:, k], r) - mI[j] * mI[k]
            if j == k:
                S[j, k] = S[j, k] + eps
    a, b, c, d, e, f = S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = (a * c00 + b * c01) + c * c02
    assert np.all(det > 0), f"guided filter: determinant {det.min()} not positive"
    i00, i01, i02, i11, i12, i22 = c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det
    inv = [[i00, i01, i02], [i01, i11, i12], [i02, i12, i22]]
    out = np.empty((p.shape[0], p.shape[1], 12) + p.shape[3:], dtype=np.float64)
    for row in range(p.shape[0]):
        for ch in range(3):
            pc = p[row, :, ch]
            bp = box(pc, r)
            cov = [box(I[:, k] * pc, r) - mI[k] * bp for k in range(3)]
            ac = [(inv[k][0] * cov[0] + inv[k][1] * cov[1]) + inv[k][2] * cov[2] for k in range(3)]
            bc = bp - ((ac[0] * mI[0] + ac[1] * mI[1]) + ac[2] * mI[2])
            for k in range(3):
                out[row, :, 3 * ch + k] = box(ac[k], r)
            out[row, :, 9 + ch] = box(bc, r)
    return out


def taps(n_full, n_low):
    """Per full-resolution coordinate P of an axis: (i0, i1, f) with v = (P + 0.5) (n_low / n_full) - 0.5 clamped to [0, n_low - 1],
    i0 = floor(v), i1 = min(i0 + 1, n_low - 1), f = v - i0."""
    ratio = np.float64(n_low) / np.float64(n_full)
    v = (np.arange(n_full, dtype=np.float64) + 0.5) * ratio
    v = v - 0.5
    v = np.minimum(np.maximum(v, 0.0), np.float64(n_low - 1))
    i0 = np.floor(v).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_low - 1)
    return i0, i1, v - i0.astype(np.float64)


def apply_one(coeffs, photo):
    """coeffs (12, hl, wl) float64, photo (h, w, 3) uint8 -> q (3, h, w) float64."""
    hl, wl = coeffs.shape[-2:]
    h, w = photo.shape[:2]
    y0, y1, fy = taps(h, hl)
    x0, x1, fx = taps(w, wl)
    fy, fx = fy[:, None], fx[None, :]
    v00, v01 = coeffs[:, y0[:, None], x0[None, :]], coeffs[:, y0[:, None], x1[None, :]]
    v10, v11 = coeffs[:, y1[:, None], x0[None, :]], coeffs[:, y1[:, None], x1[None, :]]
    top = v00 + (v01 - v00) * fx
    bot = v10 + (v11 - v10) * fx
    c = top + (bot - top) * fy
    I = photo.astype(np.float64).transpose(2, 0, 1) / 255.0
    return np.stack([((c[3 * ch] * I[0] + c[3 * ch + 1] * I[1]) + c[3 * ch + 2] * I[2]) + c[9 + ch] for ch in range(3)])


def to_bytes(q):
    """floor(clamp(q * 255, 0, 255)) as uint8: infer_driver.to_uint8's truncation."""
    return np.minimum(np.maximum(q * 255.0, 0.0), 255.0).astype(np.uint8)


def apply_batch(coeffs, photos, sizes, fill=0xA5):
    """coeffs (R, N, 12, hl, wl); photos (N, Hmax, Wmax, 3) uint8 with per-image (h, w).  Returns the padded uint8 (R, N, Hmax, Wmax, 3) with
    `fill` outside every image, and the float32 (R, N, 3, Hmax, Wmax) with NaN outside."""
    R, N = coeffs.shape[:2]
    hmax, wmax = photos.shape[1:3]
    u8 = np.full((R, N, hmax, wmax, 3), fill, dtype=np.uint8)
    f32 = np.full((R, N, 3, hmax, wmax), np.nan, dtype=np.float32)
    for n, (h, w) in enumerate(sizes):
        for row in range(R):
            q = apply_one(coeffs[row, n], photos[n, :h, :w])
            u8[row, n, :h, :w] = to_bytes(q).transpose(1, 2, 0)
            f32[row, n, :, :h, :w] = q.astype(np.float32)
    return u8, f32
