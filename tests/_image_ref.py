"""numpy restatement of the two kernels of csrc/image.hip (image_geometry_kernel with resample_coeffs_kernel, image_jitter_kernel), written
from the kernel source and Pillow's documented arithmetic (libImaging Resample.c, Geometry.c affine_fixed, Blend.c, Convert.c rgb2l,
ImageEnhance.py).  TEST INFRASTRUCTURE ONLY: it imports nothing of the HIP library and runs without a GPU.

tests/test_input_edges_cpu.py pins it byte for byte to the Pillow chain (oracle/input_ref.py) at every case of tests/_image_edge_cases.py,
so the arithmetic the kernels promise is checked at those edges on any machine; tests/test_gpu_input_edges.py then holds the kernels
themselves to Pillow.

Layout shared with the product (wu/input_pipeline.py, struct ImgGeo): a geo row is 18 int32 --
    [0:2] src_off (int64, bytes)  [2] src_h  [3] src_w  [4] src_ld (pixels)  [5] crop_top  [6] crop_left  [7] crop_h  [8] crop_w
    [9] flip  [10:16] the 16.16 affine coefficients a0..a5  [16] do_rot  [17] padding
"""
import math

import numpy as np

PREC = 22                                      # Resample.c PRECISION_BITS = 32 - 8 - 2
HALF = 1 << (PREC - 1)
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2


def ksize_for(in_size, S):
    """Resample.c precompute_coeffs: ksize = (int)ceil(support) * 2 + 1 for the bilinear filter (support 1, grown by the down-scale)."""
    return 2 * int(math.ceil(max(in_size / S, 1.0))) + 1


def coeff_table(in_size, S, ksize):
    """precompute_coeffs + normalize_coeffs_8bpc in float64 for one axis: (bounds (S, 2) = {xmin, count}, coeffs (S, ksize) int64).
    Sums run over x in order, as the C loop does (numpy's own reductions pair their terms differently)."""
    scale = float(in_size) / float(S)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    center = (np.arange(S, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)              # (int): truncation toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((S, ksize), np.float64)
    ww = np.zeros(S, np.float64)
    for x in range(ksize):
        t = np.abs((x + xmin - center + 0.5) * ss)
        w[:, x] = np.where((t < 1.0) & (x < xmax), 1.0 - t, 0.0)
        ww += w[:, x]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    q = np.where(w < 0, -0.5 + w * float(1 << PREC), 0.5 + w * float(1 << PREC)).astype(np.int64)
    q[np.arange(ksize)[None, :] >= xmax[:, None]] = 0
    return np.stack([xmin, np.minimum(xmax, ksize)], 1), q


def clip8(v):
    return np.clip(v >> PREC, 0, 255)


def rot_map(a, x, y, xsize, ysize):
    """Geometry.c affine_fixed, nearest, in C's wrapping 32-bit arithmetic: (xin, yin, inside) of the output pixels (x, y)."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    a = [int(v) for v in a]

    def c_int(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31
    xin = c_int(a[2] + a[0] * x + a[1] * y) >> 16
    yin = c_int(a[5] + a[3] * x + a[4] * y) >> 16
    return xin, yin, (xin >= 0) & (xin < xsize) & (yin >= 0) & (yin < ysize)


def geo_fields(geo_row):
    g = np.asarray(geo_row, dtype=np.int32)
    assert g.shape == (18,)
    src_off = int(g[0:2].copy().view(np.int64)[0])
    return (src_off, *(int(v) for v in g[2:10]), [int(v) for v in g[10:16]], int(g[16]))


def geometry(src_padded, geo_row, S, ksize, rot_first):
    """image_geometry_kernel for one image: (S, S, 3) uint8.  Walks backwards like the kernel: flip, [rotate the S x S result,]
    vertical taps over an 8-bit horizontal intermediate, [rotate per source tap,] the padded source buffer at stride src_ld."""
    buf = np.ascontiguousarray(src_padded).reshape(-1)
    src_off, src_h, src_w, src_ld, crop_top, crop_left, crop_h, crop_w, flip, rot, do_rot = geo_fields(geo_row)
    bx, kx = coeff_table(crop_w, S, ksize)
    by, ky = coeff_table(crop_h, S, ksize)
    # every source tap of the window, fetched the way the kernel fetches it
    sy, sx = np.mgrid[crop_top:crop_top + crop_h, crop_left:crop_left + crop_w].astype(np.int64)
    ok = np.ones(sy.shape, bool)
    ux, uy = sx, sy
    if rot_first and do_rot:
        ux, uy, ok = rot_map(rot, sx, sy, src_w, src_h)
    addr = src_off + (np.where(ok, uy, 0) * src_ld + np.where(ok, ux, 0)) * 3
    win = np.where(ok[..., None], buf[addr[..., None] + np.arange(3)], 0).astype(np.int64)        # (crop_h, crop_w, 3)
    # horizontal pass to the 8-bit intermediate, one column of the S-wide result at a time
    hor = np.empty((crop_h, S, 3), np.int64)
    for px in range(S):
        x0, nx = int(bx[px, 0]), int(bx[px, 1])
        hor[:, px] = clip8(HALF + np.tensordot(win[:, x0:x0 + nx], kx[px, :nx], axes=([1], [0])))
    res = np.empty((S, S, 3), np.int64)
    for py in range(S):
        y0, ny = int(by[py, 0]), int(by[py, 1])
        res[py] = clip8(HALF + np.tensordot(ky[py, :ny], hor[y0:y0 + ny], axes=([0], [0])))
    # output pixel -> pixel of the resized image
    oy, ox = np.mgrid[0:S, 0:S].astype(np.int64)
    px, py = (S - 1 - ox if flip else ox), oy
    inside = np.ones((S, S), bool)
    if not rot_first and do_rot:
        px, py, inside = rot_map(rot, px, py, S, S)
    out = np.where(inside[..., None], res[np.where(inside, py, 0), np.where(inside, px, 0)], 0)   # Image.rotate fills with black
    return out.astype(np.uint8)


def grey_l(img):
    """Convert.c rgb2l on an (..., 3) integer array."""
    v = img.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def blend8(degenerate, v, alpha, fused=False):
    """Blend.c: degenerate + alpha * (v - degenerate) in C float, truncated to a byte (clipped first when alpha is outside [0, 1]).
    fused=False: the product and the sum are each rounded to float32 (what Pillow computes); fused=True: one rounding of the exact
    result, what a fused multiply-add gives.  The exact result fits float64: a 24-bit factor times a 9-bit difference, plus a byte."""
    alpha = np.float32(alpha)
    d32, v32 = np.asarray(degenerate).astype(np.float32), np.asarray(v).astype(np.float32)
    if fused:
        t = (d32.astype(np.float64) + np.float64(alpha) * (v32.astype(np.float64) - d32.astype(np.float64))).astype(np.float32)
    else:
        prod = (alpha * (v32 - d32)).astype(np.float32)
        t = (d32 + prod).astype(np.float32)
    if 0.0 <= alpha <= 1.0:
        return t.astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


def jitter(img_u8, factors, order, fused=False):
    """image_jitter_kernel for one (S, S, 3) uint8 image: ImageEnhance.Brightness / Contrast / Color in the given order (entries
    outside 0..2 are skipped)."""
    img = np.array(img_u8, dtype=np.uint8)
    npix = img.shape[0] * img.shape[1]
    for op in order:
        if op < 0 or op > 2:
            continue
        f = np.float32(factors[op])
        if op == BRIGHTNESS:
            d = np.zeros(img.shape, np.int64)
        elif op == CONTRAST:
            d = np.full(img.shape, int(float(grey_l(img).sum()) / float(npix) + 0.5), np.int64)
        else:
            d = np.broadcast_to(grey_l(img)[..., None], img.shape)
        img = blend8(d, img, f, fused)
    return img


def normalize(hwc_u8):
    """ToTensor + Normalize(0.5, 0.5) in float32, as the kernels' epilogue does it: (v / 255 - 0.5) / 0.5, CHW."""
    t = hwc_u8.astype(np.float32) / np.float32(255.0)
    t = (t - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(t.transpose(2, 0, 1))


def rotate_coeffs(angle_deg, w, h):
    """Image.rotate(angle, NEAREST, expand=False, center=None) as 16.16 coefficients (restated here so the module stands alone;
    test_input_edges_cpu.py holds it equal to wu.input_pipeline.rotate_coeffs)."""
    a = -math.radians(angle_deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy

    def fix(v):
        v = v * 65536.0 + 0.5
        return int(math.floor(v)) if v < 0.0 else int(v)
    out = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    return [((v + 2 ** 31) % 2 ** 32) - 2 ** 31 for v in out]


def geo_rows(shape, sizes, params, S, rot_first, train=True):
    """The (N, 18) int32 table and the batch ksize GPUInputPipeline.__call__ builds for a (N, Hmax, Wmax, 3) buffer."""
    n, hmax, wmax, _ = shape
    geo = np.zeros((n, 18), np.int32)
    ksize = 3
    for i, ((h, w), p) in enumerate(zip(sizes, params)):
        ct, cl, ch, cw = p["crop"]
        geo[i, 0:2] = np.array([i * hmax * wmax * 3], np.int64).view(np.int32)
        geo[i, 2:9] = (h, w, wmax, ct, cl, ch, cw)
        geo[i, 9] = 1 if p["flip"] else 0
        do_rot = bool(train) and p["angle"] % 360.0 != 0.0
        if do_rot:
            geo[i, 10:16] = rotate_coeffs(p["angle"], w if rot_first else S, h if rot_first else S)
        geo[i, 16] = 1 if do_rot else 0
        ksize = max(ksize, ksize_for(ch, S), ksize_for(cw, S))
    return geo, ksize


def pipeline(src_padded, sizes, params, S, augmentation, train, fused=False):
    """The whole batch transform, host table + both kernels: (N, 3, S, S) float32 and the (N, S, S, 3) uint8 image before Normalize."""
    rot_first = bool(train and augmentation)
    geo, ksize = geo_rows(src_padded.shape, sizes, params, S, rot_first, train)
    u8 = np.stack([geometry(src_padded, geo[i], S, ksize, rot_first) for i in range(len(sizes))])
    for i, p in enumerate(params):
        if any(o >= 0 for o in p["order"]):
            u8[i] = jitter(u8[i], p["factors"], p["order"], fused)
    return np.stack([normalize(im) for im in u8]), u8
