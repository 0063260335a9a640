"""numpy restatement of the baseline JPEG encoder of csrc/jpeg_enc.hip: libjpeg's default compress path as Pillow runs it for
``Image.fromarray(rgb).save(f, 'JPEG', quality=q, subsampling=s)`` -- Annex K tables scaled by quality, 16.16 fixed-point RGB -> YCbCr,
h2v2 chroma downsampling with libjpeg's asymmetric edge padding, the "islow" forward DCT, quantisation by true integer division, dummy
blocks, the standard Huffman tables, byte stuffing.  Test infrastructure only: slow, exact, staged (``stages`` returns every
intermediate the kernels produce so that a GPU mismatch can be pinned to its stage)."""
import io

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                     99, 99] + [99] * 32)
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))

SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (15, 16), (16, 16), (17, 17), (24, 40), (40, 24), (33, 1), (3, 40), (64, 48), (100, 75)]
EXTRA_SIZES = [(12, 12), (50, 16), (4, 4)]
GPU_SIZES = [(1, 1), (7, 5), (8, 8), (12, 12), (16, 16), (17, 17), (24, 40), (40, 24), (33, 1), (3, 40), (50, 16), (100, 75)]
CONTENTS = ("noise", "gradient", "flat", "saturated")
QUALITIES = (None, 100, 30)          # None: Pillow's default (75)


def make_image(h, w, content, seed=0):
    """(h, w, 3) uint8 test image; deterministic in (h, w, content, seed)."""
    rng = np.random.default_rng([h, w, CONTENTS.index(content), seed])
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(h + w - 2, 1)], axis=-1)
        return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
    if content == "flat":
        return np.broadcast_to(np.array([200, 31, 97], dtype=np.uint8), (h, w, 3)).copy()
    # saturated: a coarse random pattern of pure 0 / 255 samples -- the largest DC differences and coefficients 8-bit input can make
    cells = rng.integers(0, 2, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8) * 255
    img = np.repeat(np.repeat(cells, 8, axis=0), 8, axis=1)[:h, :w].copy()
    flip = rng.random((h, w, 3)) < 0.05
    img[flip] = 255 - img[flip]
    return img


def pillow_jpeg(rgb, quality=None, subsampling=None):
    """The bytes Image.save writes; quality None / subsampling None = Pillow's defaults (75, 4:2:0)."""
    from PIL import Image
    kw = {}
    if quality is not None:
        kw["quality"] = quality
    if subsampling is not None:
        kw["subsampling"] = subsampling
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def quant_tables(quality):
    """(luma, chroma) int arrays in natural order: jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)."""
    q = 75 if quality is None else int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def _segment(marker, body):
    return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)


def header(h, w, quality=None, subsampling="4:2:0"):
    """SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS -- everything in front of the entropy-coded data."""
    ql, qc = quant_tables(quality)
    samp = {"4:2:0": 0x22, "4:4:4": 0x11}[subsampling]
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, [0] + [int(v) for v in ql[ZIGZAG]]) + _segment(0xDB, [1] + [int(v) for v in qc[ZIGZAG]])
    out += _segment(0xC0, [8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, samp, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                              (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _segment(0xC4, [tc_th] + bits + vals)
    return out + _segment(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def huff_codes(bits, vals):
    """symbol -> (code, length) of a JPEG Huffman table (Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    """jccolor.c rgb_ycc_convert: three int planes."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + 32768) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_edge(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def component_planes(rgb, subsampling="4:2:0"):
    """The three sample planes padded to whole MCUs exactly as jcprepct / jcsample leave them."""
    h, w = rgb.shape[:2]
    y, cb, cr = rgb_to_ycc(rgb)
    if subsampling == "4:4:4":
        H, W = -(-h // 8) * 8, -(-w // 8) * 8
        return [_pad_edge(p, H, W) for p in (y, cb, cr)]
    H, W = -(-h // 16) * 16, -(-w // 16) * 16
    planes = [_pad_edge(y, H, W)]
    bias = np.tile(np.array([1, 2]), W // 4 + 1)[:W // 2]
    for c in (cb, cr):
        full = _pad_edge(c, h + (h & 1), W)          # right: the last full-resolution column; bottom: only to complete a row pair
        down = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
        planes.append(_pad_edge(down, H // 2, W // 2))          # below that: the last DOWNSAMPLED row
    return planes


def _fdct_pass(d, first):
    """One 1-D pass of jfdctint.c (jpeg_fdct_islow) along the last axis."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    sh = 11 if first else 15

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2], out[..., 6] = descale(z1 + t13 * 6270, sh), descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7], out[..., 5], out[..., 3], out[..., 1] = (descale(t4 + z1 + z3, sh), descale(t5 + z2 + z4, sh), descale(t6 + z2 + z3, sh),
                                                          descale(t7 + z1 + z4, sh))
    return out


def fdct_quant(plane, qtab):
    """plane (8*bh, 8*bw) samples -> (bh, bw, 64) quantised coefficients in ZIGZAG order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    rows = _fdct_pass(blocks, True)                                                   # rows first
    coef = _fdct_pass(rows.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)        # then columns
    div = (8 * qtab.astype(np.int64)).reshape(8, 8)
    q = np.sign(coef) * ((np.abs(coef) + (div >> 1)) // div)
    return q.reshape(bh, bw, 64)[..., ZIGZAG]


def scan_blocks(rgb, quality=None, subsampling="4:2:0"):
    """Quantised blocks in scan order with their component: (nblocks, 64) int array (zigzag), (nblocks,) component ids.  Dummy blocks
    (jccoefct.c compress_data) are materialised: AC zero, DC of the previous block in MCU order."""
    h, w = rgb.shape[:2]
    ql, qc = quant_tables(quality)
    planes = component_planes(rgb, subsampling)
    coefs = [fdct_quant(planes[0], ql), fdct_quant(planes[1], qc), fdct_quant(planes[2], qc)]
    out, comp = [], []
    if subsampling == "4:4:4":
        for my in range(coefs[0].shape[0]):
            for mx in range(coefs[0].shape[1]):
                for c in range(3):
                    out.append(coefs[c][my, mx])
                    comp.append(c)
        return np.array(out), np.array(comp)
    bw_real, bh_real = -(-w // 8), -(-h // 8)
    for my in range(coefs[1].shape[0]):
        for mx in range(coefs[1].shape[1]):
            for k in range(4):
                by, bx = 2 * my + (k >> 1), 2 * mx + (k & 1)
                if by < bh_real and bx < bw_real:
                    blk = coefs[0][by, bx]
                else:
                    blk = np.zeros(64, dtype=np.int64)
                    blk[0] = out[-1][0]
                out.append(blk)
                comp.append(0)
            for c in (1, 2):
                out.append(coefs[c][my, mx])
                comp.append(c)
    return np.array(out), np.array(comp)


def _category(v):
    return int(abs(int(v))).bit_length()


def encode_blocks(blocks, comp):
    """Huffman-encode scan-order blocks: (list of per-block bit strings)."""
    dc = [huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS)]
    ac = [huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    pred = [0, 0, 0]
    out = []

    def put(bits, code, length):
        bits.append(format(code, "b").zfill(length) if length else "")

    def magnitude(bits, v, n):
        if n:
            put(bits, (int(v) if v > 0 else int(v) - 1) & ((1 << n) - 1), n)
    for blk, c in zip(blocks, comp):
        t = 0 if c == 0 else 1
        bits = []
        diff = int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
        n = _category(diff)
        put(bits, *dc[t][n])
        magnitude(bits, diff, n)
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(bits, *ac[t][0xF0])
                run -= 16
            n = _category(v)
            put(bits, *ac[t][(run << 4) | n])
            magnitude(bits, v, n)
            run = 0
        if run:
            put(bits, *ac[t][0x00])
        out.append("".join(bits))
    return out


def stages(rgb, quality=None, subsampling="4:2:0"):
    """Every intermediate: dict(blocks (nb, 64) zigzag, comp, bits (nb,) per-block bit counts, raw (unstuffed scan bytes, final byte
    padded with ones), scan (stuffed), file)."""
    rgb = np.asarray(rgb)
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.dtype == np.uint8
    blocks, comp = scan_blocks(rgb, quality, subsampling)
    strings = encode_blocks(blocks, comp)
    stream = "".join(strings)
    stream += "1" * (-len(stream) % 8)
    raw = int(stream, 2).to_bytes(len(stream) // 8, "big") if stream else b""
    scan = raw.replace(b"\xff", b"\xff\x00")
    return {"blocks": blocks, "comp": comp, "bits": np.array([len(s) for s in strings]), "raw": raw, "scan": scan,
            "file": header(rgb.shape[0], rgb.shape[1], quality, subsampling) + scan + b"\xff\xd9"}


def encode(rgb, quality=None, subsampling="4:2:0"):
    """The complete JPEG file."""
    return stages(rgb, quality, subsampling)["file"]

