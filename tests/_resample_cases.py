"""The cases of the resampling tests (tests/test_resample_cpu.py, tests/test_gpu_resample.py): ragged batches grouped by output size,
their pictures (noise plus 0 / 255 stripes), the poisoned padded batch the device reads, and Pillow's answer.

The (h, w) -> (oh, ow) shapes: a 2.3x / 3.3x and a 12.9x / 17.2x down-scale, an up-scale, a 1 x 1 source, one pass skipped on either axis,
both passes skipped, a 21x down-scale to 3 x 3, a 1 x 1 output, a 128.9x down-scale on one axis (517 taps), and a stripe picture that
bicubic and Lanczos take outside [0, 255] in float mode.  Every batch holds images of different sizes; output heights 1, 5, 29 and 31
(none a multiple of 3) serve the band tests."""
import numpy as np

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
MODES = ("u8", "f32")

# name -> ((oh, ow), [(h, w, kind)]); kind: "mixed" = noise with a striped region, "stripes" = 0 / 255 stripes only
BATCHES = {
    "down_16": ((16, 16), [(37, 53, "mixed"), (16, 20, "mixed")]),
    "photo_29": ((29, 29), [(375, 500, "mixed"), (31, 29, "mixed")]),
    "up_29x31": ((29, 31), [(7, 5, "mixed"), (29, 31, "mixed"), (12, 16, "stripes")]),
    "pixel_4": ((4, 4), [(1, 1, "mixed"), (3, 7, "mixed")]),
    "hpass_40x13": ((40, 13), [(40, 40, "mixed"), (11, 13, "mixed")]),
    "hpass_13x9": ((13, 9), [(13, 200, "mixed"), (5, 4, "mixed")]),
    "vpass_5x17": ((5, 17), [(300, 17, "mixed"), (6, 40, "stripes")]),
    "down_3": ((3, 3), [(64, 64, "mixed"), (2, 5, "mixed")]),
    "down_1": ((1, 1), [(9, 9, "mixed"), (1, 3, "mixed")]),
    "steep_20x30": ((20, 30), [(20, 3867, "mixed"), (33, 30, "mixed")]),
    "band_31x29": ((31, 29), [(50, 40, "mixed"), (31, 47, "stripes")]),
}
SMALL, STEEP = "down_16", "steep_20x30"                           # the workspace test's two batches
BAND_BATCHES = ("down_1", "vpass_5x17", "photo_29", "band_31x29")   # output heights 1, 5, 29, 31
OVERSHOOT = ("up_29x31", 2)                                       # the stripe picture whose float-mode output leaves [0, 255]


def picture(h, w, kind, seed):
    """(h, w, 3) uint8."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "stripes":
        img[:] = (255 * (((xx // 2) + (yy // 3)) % 2))[:, :, None].astype(np.uint8)
    else:
        right = xx >= w // 2
        img[right] = (255 * ((xx + yy) % 2))[right][:, None].astype(np.uint8)
    return img


def pictures(name):
    size, items = BATCHES[name]
    seed = sorted(BATCHES).index(name) * 16
    return [picture(h, w, kind, seed + i) for i, (h, w, kind) in enumerate(items)]


def padded(images, fill, margin=3):
    """((N, Hmax + margin, Wmax + margin, 3) uint8, [(h, w)]): the padding is 255 or noise, never what an image holds at its edge."""
    hm = max(a.shape[0] for a in images) + margin
    wm = max(a.shape[1] for a in images) + margin
    if fill == "255":
        host = np.full((len(images), hm, wm, 3), 255, dtype=np.uint8)
    else:
        host = np.random.default_rng(99).integers(0, 256, (len(images), hm, wm, 3), dtype=np.uint8)
    for k, a in enumerate(images):
        host[k, :a.shape[0], :a.shape[1]] = a
    return host, [(a.shape[0], a.shape[1]) for a in images]


def pillow(img, size, name, mode):
    """Image.resize of the RGB uint8 image (mode "u8"), or of each channel as a mode 'F' image (mode "f32": (oh, ow, 3) float32)."""
    from PIL import Image
    resample = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]
    oh, ow = size
    if mode == "u8":
        return np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), resample))
    chans = [np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, c].astype(np.float32)), "F").resize((ow, oh), resample)) for c in range(3)]
    return np.stack(chans, axis=2).astype(np.float32)


_WANT = {}


def want(name, filt, mode):
    """Pillow's answers for a batch, computed once: [(oh, ow, 3)] per image."""
    key = (name, filt, mode)
    if key not in _WANT:
        size = BATCHES[name][0]
        _WANT[key] = [pillow(a, size, filt, mode) for a in pictures(name)]
    return _WANT[key]


def dump(directory):
    """Every batch x filter x mode as files for scratch/resample_emu.cpp.  NAME.in: int32 N, Hout, Wout, mode (1 = 8-bit), Hmax, Wmax and
    the workspace image's byte count, then that image (wu.resample.GPUResampler.plan: descriptors + tables) and the noise-padded uint8
    source; NAME.want: Pillow's (N, Hout, Wout, 3) uint8 or float32.  Returns the number of cases."""
    import os
    from wu.resample import GPUResampler
    os.makedirs(directory, exist_ok=True)
    count = 0
    for name in sorted(BATCHES):
        (oh, ow), _ = BATCHES[name]
        host, sizes = padded(pictures(name), "noise")
        n, hm, wm, _ = host.shape
        for filt in FILTERS:
            for mode in MODES:
                _, image = GPUResampler((oh, ow), filt, mode, "nhwc_u8" if mode == "u8" else "raw").plan(sizes, (hm * wm * 3, wm * 3, 3, 1))
                head = np.array([n, oh, ow, 1 if mode == "u8" else 0, hm, wm, len(image)], dtype=np.int32)
                base = os.path.join(directory, f"{name}.{filt}.{mode}")
                with open(base + ".in", "wb") as fh:
                    fh.write(head.tobytes() + image + host.tobytes())
                with open(base + ".want", "wb") as fh:
                    fh.write(np.stack(want(name, filt, mode)).tobytes())
                count += 1
    return count


def bits(a):
    """The bit patterns of a float32 array (so that -0.0 / 0.0 and NaNs compare as what they are)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
