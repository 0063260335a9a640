"""Numpy restatement of the reconstruction half of a baseline JPEG decode, as libjpeg's default path (= Pillow) computes it:
dequantisation, jidctint's "islow" 8x8 IDCT, "fancy" h2v1 / h2v2 chroma upsampling on the component's true down-sampled size
(plain replication when that width is <= 2), jdcolor's fixed-point YCbCr -> RGB.  No Huffman code: it consumes what
wu.jpeg.entropy_decode returns.  Test infrastructure (like _inception_ref.py), plus the image generators the JPEG tests share."""
import io

import numpy as np

C = dict(F0298=2446, F0390=3196, F0541=4433, F0765=6270, F0899=7373, F1175=9633, F1501=12299, F1847=15137, F1961=16069, F2053=16819,
         F2562=20995, F3072=25172)


def idct_pass(i0, i1, i2, i3, i4, i5, i6, i7, shift):
    z2, z3 = i2, i6
    z1 = (z2 + z3) * C["F0541"]
    tmp2 = z1 + z3 * (-C["F1847"])
    tmp3 = z1 + z2 * C["F0765"]
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i7, i5, i3, i1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * C["F1175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * C["F0298"], tmp1 * C["F2053"], tmp2 * C["F3072"], tmp3 * C["F1501"]
    z1, z2, z3, z4 = z1 * -C["F0899"], z2 * -C["F2562"], z3 * -C["F1961"], z4 * -C["F0390"]
    z3 = z3 + z5
    z4 = z4 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4

    def d(x):
        return (x + (1 << (shift - 1))) >> shift
    return [d(tmp10 + tmp3), d(tmp11 + tmp2), d(tmp12 + tmp1), d(tmp13 + tmp0), d(tmp13 - tmp0), d(tmp12 - tmp1), d(tmp11 - tmp2), d(tmp10 - tmp3)]


def idct(blocks, qt):
    """blocks (..., 64) quantised coefficients in natural order, qt (64,) -> (..., 8, 8) samples 0..255"""
    x = (blocks.astype(np.int64) * qt.astype(np.int64)).reshape(blocks.shape[:-1] + (8, 8))
    ws = np.stack(idct_pass(*[x[..., r, :] for r in range(8)], 11), axis=-2)        # pass 1: down the columns
    out = np.stack(idct_pass(*[ws[..., :, c] for c in range(8)], 18), axis=-1)      # pass 2: along the rows
    return np.clip(out + 128, 0, 255).astype(np.int32)


def plane(pl, qt):
    by, bx, _ = pl.shape
    return idct(pl, qt).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def up_h2v1(p, dw):
    p = p[:, :dw]
    if dw <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.zeros((p.shape[0], 2 * dw), np.int32)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def up_h2v2(p, dw, dh):
    p = p[:dh, :dw]
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    out = np.zeros((2 * dh, 2 * dw), np.int32)
    for v, nb in ((0, above), (1, below)):
        cs = 3 * p + nb
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[v::2, 0::2] = (3 * cs + left + 8) >> 4
        out[v::2, 1::2] = (3 * cs + right + 7) >> 4
        out[v::2, 0] = (4 * cs[:, 0] + 8) >> 4
        out[v::2, -1] = (4 * cs[:, -1] + 7) >> 4
    return out


def reconstruct(decoded):
    """decoded = wu.jpeg.entropy_decode(data) = (planes, qtabs, info) -> (H, W, 3) uint8 RGB"""
    planes, qtabs, info = decoded
    H, W = info.height, info.width
    px = [plane(pl, qtabs[c]) for c, pl in enumerate(planes)]
    if len(planes) == 1:
        y = px[0][:H, :W]
        return np.stack([y, y, y], -1).astype(np.uint8)
    hmax, vmax = info.hs[0], info.vs[0]
    dw, dh = -(-W // hmax), -(-H // vmax)
    full = [px[0]]
    for ci in (1, 2):
        if (hmax, vmax) == (1, 1):
            full.append(px[ci])
        elif (hmax, vmax) == (2, 1):
            full.append(up_h2v1(px[ci], dw))
        elif (hmax, vmax) == (2, 2):
            full.append(up_h2v2(px[ci], dw, dh))
        else:
            raise ValueError("sampling")
    y, cb, cr = [f[:H, :W].astype(np.int64) for f in full]

    def fix(x):
        return int(x * 65536 + 0.5)
    r = y + ((fix(1.40200) * (cr - 128) + 32768) >> 16)
    g = y + ((-fix(0.34414) * (cb - 128) + 32768 - fix(0.71414) * (cr - 128)) >> 16)
    b = y + ((fix(1.77200) * (cb - 128) + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- shared test images ---------------------------------------------------------------------------------------------------------
SMALL_SIZES = [(97, 131), (64, 48), (33, 17), (16, 16), (8, 8), (7, 5), (1, 1), (3, 40), (40, 3), (120, 161), (18, 34)]
LARGE_SIZES = [(375, 500), (500, 333), (600, 800), (224, 224)]          # the sizes of test_gpu_input.py
VARIANTS = [("q75_420", dict(quality=75)), ("q90_444", dict(quality=90, subsampling=0)), ("q85_422", dict(quality=85, subsampling=1)),
            ("q100_420", dict(quality=100, subsampling=2)), ("q30_rst3", dict(quality=30, restart_marker_blocks=3)),
            ("q75_opt", dict(quality=75, optimize=True)), ("q5", dict(quality=5)), ("grey", "grey"),
            ("q95_422", dict(quality=95, subsampling=1)), ("q85_420", dict(quality=85, subsampling=2)),
            ("q30_444_rst1", dict(quality=30, subsampling=0, restart_marker_blocks=1)), ("q75_rstrow", dict(quality=75, restart_marker_rows=1)),
            ("q100_444", dict(quality=100, subsampling=0))]


def synth(h, w, seed):
    """Smooth structure + noise, in the style of test_gpu_input.py::_batch."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + seed), 128 + 90 * np.cos(yy / 5.0), 40 + (xx + yy) % 200], -1)
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(img, kw):
    from PIL import Image
    f = io.BytesIO()
    if kw == "grey":
        Image.fromarray(img[..., 1]).save(f, "JPEG", quality=80)
    else:
        Image.fromarray(img).save(f, "JPEG", **kw)
    return f.getvalue()


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def grid(sizes=None, variants=None):
    """[(name, jpeg bytes)] over sizes x variants."""
    out = []
    for si, (h, w) in enumerate(SMALL_SIZES if sizes is None else sizes):
        img = synth(h, w, si)
        for name, kw in (VARIANTS if variants is None else variants):
            out.append((f"{h}x{w}_{name}", encode(img, kw)))
    return out
