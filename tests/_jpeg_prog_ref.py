"""What the progressive / 4:4:0 tests share on top of _jpeg_ref.py: the numpy restatement of libjpeg-turbo's h1v2 "fancy" chroma
up-sampling (the one mode _jpeg_ref.reconstruct lacks), and the fixtures -- all written live by Pillow:

  * a progressive file and its BASELINE TWIN (the same arguments without ``progressive``) hold the same quantised coefficients, so the
    twin's entropy_decode is the exact oracle of the progressive scans;
  * a 4:4:0 file is a 4:2:2 file of a SQUARE picture with the luma sampling byte patched 0x21 -> 0x12 (the MCU and block counts agree at
    every square size; it is a valid file of another picture), and Pillow's decode of the patched bytes is the oracle;
  * an INCOMPLETE progressive file is a progressive file cut at an SOS boundary with EOI appended.
Test infrastructure; no Huffman code here."""
import numpy as np

import _jpeg_ref as R

# the cases of the issue: every SMALL_SIZES size times these
PROG_VARIANTS = [("q75_420", dict(quality=75)), ("q90_444", dict(quality=90, subsampling=0)), ("q85_422", dict(quality=85, subsampling=1)),
                 ("grey", "grey"), ("q5", dict(quality=5)), ("q100_420", dict(quality=100, subsampling=2)),
                 ("q30_rst3", dict(quality=30, restart_marker_blocks=3)), ("q30_444_rst1", dict(quality=30, subsampling=0, restart_marker_blocks=1)),
                 ("q75_rstrow", dict(quality=75, restart_marker_rows=1)), ("q75_opt", dict(quality=75, optimize=True))]
SQUARE_440 = [1, 2, 7, 8, 16, 17, 33, 48, 97]


def encode(img, kw, progressive):
    """R.encode with ``progressive=True`` added (grey: the luma subset of the same script)."""
    if not progressive:
        return R.encode(img, kw)
    if kw == "grey":
        import io
        from PIL import Image
        f = io.BytesIO()
        Image.fromarray(img[..., 1]).save(f, "JPEG", quality=80, progressive=True)
        return f.getvalue()
    return R.encode(img, dict(kw, progressive=True))


def twins(size, seed, variants=None):
    """[(name, progressive bytes, baseline twin bytes)] of one picture over the variants."""
    img = R.synth(size[0], size[1], seed)
    return [(f"{size[0]}x{size[1]}_{name}", encode(img, kw, True), encode(img, kw, False)) for name, kw in (PROG_VARIANTS if variants is None else variants)]


def sof_at(data):
    for m in (b"\xff\xc0", b"\xff\xc2"):
        if m in data:
            return data.index(m)
    raise ValueError("no SOF0 / SOF2")


def make_440(side, seed=9, progressive=False, quality=80):
    """A 4:4:0 file of side x side: Pillow's 4:2:2 with the luma sampling byte patched."""
    data = encode(R.synth(side, side, seed), dict(quality=quality, subsampling=1), progressive)
    at = sof_at(data)
    assert data[at + 11] == 0x21
    return data[:at + 11] + b"\x12" + data[at + 12:]


def sos_offsets(data):
    """Byte offsets of the SOS markers, found by walking the segments (entropy-coded data never holds 0xFF 0xDA: 0xFF is stuffed)."""
    out, pos = [], 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        m = data[pos + 1]
        if m == 0xD9:
            break
        if m == 0xDA:
            out.append(pos)
            pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
            continue
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return out


def make_incomplete(data, keep_scans):
    """The first ``keep_scans`` scans of a progressive file, then EOI: a valid file that stops short of full precision."""
    sos = sos_offsets(data)
    assert 0 < keep_scans < len(sos)
    return data[:sos[keep_scans]] + b"\xff\xd9"


def up_h1v2(p, dw, dh):
    """jdsample.c h1v2_fancy_upsample: each chroma row becomes two; the upper is 3/4 this row + 1/4 the row above (+1), the lower
    3/4 this row + 1/4 the row below (+2), >> 2; the rows beyond the component's true height are the edge rows.  Any width."""
    p = p[:dh, :dw]
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    out = np.zeros((2 * dh, dw), np.int32)
    out[0::2] = (3 * p + above + 1) >> 2
    out[1::2] = (3 * p + below + 2) >> 2
    return out


def colour(y, cb, cr):
    y, cb, cr = [f.astype(np.int64) for f in (y, cb, cr)]

    def fix(x):
        return int(x * 65536 + 0.5)
    r = y + ((fix(1.40200) * (cr - 128) + 32768) >> 16)
    g = y + ((-fix(0.34414) * (cb - 128) + 32768 - fix(0.71414) * (cr - 128)) >> 16)
    b = y + ((fix(1.77200) * (cb - 128) + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def reconstruct(decoded):
    """_jpeg_ref.reconstruct plus luma sampling 1x2."""
    planes, qtabs, info = decoded
    if len(planes) == 3 and (info.hs[0], info.vs[0]) == (1, 2):
        H, W = info.height, info.width
        px = [R.plane(pl, qtabs[c]) for c, pl in enumerate(planes)]
        full = [px[0]] + [up_h1v2(px[ci], W, -(-H // 2)) for ci in (1, 2)]
        return colour(*[f[:H, :W] for f in full])
    return R.reconstruct(decoded)
