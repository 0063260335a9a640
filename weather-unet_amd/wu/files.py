"""Image files to GPU batches: the one reader behind the metric and baseline commands (wu.fid, wu.swd, wu.paired, wu.lpips, wu.colour,
wu.retrieval).  Listing a directory, opening a file with Pillow, making and closing the JPEG / PNG decoder of a pass and padding a ragged
batch happen here and nowhere else in those modules (but for wu.retrieval's figure cells, which Pillow resizes before they are arrays).

Importing this module needs no GPU and loads no kernel library: the decoders, the input pipeline and the resampler are imported by the
functions that use them."""
import contextlib
import os
import pathlib

import numpy as np

# Two listing rules, on purpose.  The metrics of two UNPAIRED sets (FID / KID / PRDC, SWD, retrieval, the colour palettes) list a directory
# as pytorch-fid's fid_score.py does: *.jpg and *.png, case-sensitive, as Path objects.  The PAIRED metrics (SSIM, LPIPS) pair two
# directories by file stem, and a partner may have been written by another tool: .jpg / .jpeg / .png in either case, as str paths.
_EXTENSIONS = (".jpg", ".jpeg", ".png")


def image_files(path):
    p = pathlib.Path(path)
    return sorted(list(p.glob("*.jpg")) + list(p.glob("*.png")))


def _by_stem(d):
    out = {}
    for name in sorted(os.listdir(d)):
        stem, ext = os.path.splitext(name)
        if ext.lower() in _EXTENSIONS:
            if stem in out:
                raise ValueError(f"pair_files: {d} holds two images with the stem {stem!r}")
            out[stem] = os.path.join(d, name)
    return out


def pair_files(dir_a, dir_b):
    """[(path_a, path_b)] of the .jpg / .jpeg / .png files of two directories paired by file stem, sorted; ValueError listing the files
    without a partner."""
    a, b = _by_stem(dir_a), _by_stem(dir_b)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    if only_a or only_b:
        raise ValueError(f"pair_files: unpaired files -- only in {dir_a}: {[os.path.basename(a[s]) for s in only_a]}; "
                         f"only in {dir_b}: {[os.path.basename(b[s]) for s in only_b]}")
    if not a:
        raise ValueError(f"pair_files: no .jpg / .jpeg / .png files in {dir_a}")
    return [(a[s], b[s]) for s in sorted(a)]


def read_rgb(path):
    """One file through Pillow: (h, w, 3) uint8."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def same_size(sizes, where, then=""):
    """ValueError ``images of different sizes <where><the sorted set of sizes><then>`` unless every (h, w) of ``sizes`` is the same."""
    distinct = sorted(set((int(h), int(w)) for h, w in sizes))
    if len(distinct) > 1:
        raise ValueError(f"images of different sizes {where}{distinct}{then}")


# ----------------------------------------------------------------------------------------------
# files -> padded batches -> resampled batches
# ----------------------------------------------------------------------------------------------
def padded_host(arrays):
    """(h, w, 3) uint8 arrays of any sizes -> ((N, Hmax, Wmax, 3) uint8 numpy array, zero padded, [(h, w)]).  Arrays of one size come
    out as ``np.stack`` of them."""
    sizes = [(int(a.shape[0]), int(a.shape[1])) for a in arrays]
    hm, wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
    host = np.zeros((len(arrays), hm, wm, 3), dtype=np.uint8)
    for k, a in enumerate(arrays):
        host[k, :a.shape[0], :a.shape[1]] = a
    return host, sizes


def padded_batch(arrays, device):
    """``padded_host`` uploaded: ((N, Hmax, Wmax, 3) uint8 CUDA tensor, [(h, w)])."""
    import torch
    host, sizes = padded_host(arrays)
    return torch.from_numpy(host).to(device), sizes


@contextlib.contextmanager
def pass_decoder(gpu_decode=False, gpu_decode_png=False, gpu_entropy=False, gpu_extended=False):
    """The decoder of one pass over a directory, closed on every way out: a wu.png.GPUPngDecoder with ``gpu_decode_png``, else a
    wu.jpeg.GPUJpegDecoder with ``gpu_decode`` or ``gpu_entropy`` (which implies it and selects ``entropy="device"``) or ``gpu_extended``
    (which implies it too and selects ``coverage="extended"``: progressive and 4:4:0 files natively; not with ``gpu_entropy``), else
    None: Pillow."""
    dec = None
    if gpu_decode_png:
        from .png import GPUPngDecoder
        dec = GPUPngDecoder()
    elif gpu_decode or gpu_entropy or gpu_extended:
        from .jpeg import GPUJpegDecoder
        dec = GPUJpegDecoder(entropy="device" if gpu_entropy else "host", coverage="extended" if gpu_extended else "baseline")
    try:
        yield dec
    finally:
        if dec is not None:
            dec.close()


def read_batches(files, batch_size, decoder=None, device="cuda"):
    """Generator of (padded uint8 batch, [(h, w)]) over ``files``: through ``decoder.decode_batch`` (a GPUJpegDecoder / GPUPngDecoder) when
    one is given, through Pillow otherwise -- the same padded batch either way."""
    for i in range(0, len(files), batch_size):
        part = files[i:i + batch_size]
        if decoder is not None:
            batch, sizes = decoder.decode_batch(part)
            yield batch, [(int(h), int(w)) for h, w in sizes]
        else:
            yield padded_batch([read_rgb(f) for f in part], device)


def resize_files(files, size, filter="bicubic", mode="f32", out="nchw", batch_size=64, decoder=None, device="cuda", band=None):
    """Generator over ``files``: each batch read (``read_batches``) and resized to ``size`` by one GPUResampler."""
    from .resample import GPUResampler
    rs = GPUResampler(size, filter, mode, out, band)
    for batch, sizes in read_batches(files, batch_size, decoder, device):
        yield rs(batch, sizes)


def read_images(files, size=None, gpu_decode=False, device="cuda:0", batch_size=64, filter=None, gpu_extended=False):
    """Generator of (x, value_range) over ``files``, every x of one image size.  Without ``size``: the uint8 NHWC batch as an NCHW view
    (read through its strides) with the range ``"uint8"``; a batch of mixed sizes raises.  With ``size``: (N, 3, S, S) float32 in
    ``(-1, 1)`` from wu.input_pipeline (its bilinear resize), or with ``filter`` too from wu.resample with that Pillow filter in 8-bit
    mode.  ``gpu_decode``: read through wu.jpeg.GPUJpegDecoder, closed when the generator ends or is abandoned; ``gpu_extended``: the
    same with ``coverage="extended"``."""
    if filter is not None and not size:
        raise ValueError("--filter chooses how --size resizes: give --size")
    with pass_decoder(gpu_decode, gpu_extended=gpu_extended) as dec:
        if filter is not None:
            for x in resize_files(files, size, filter, "u8", "nchw", batch_size, dec, device):
                yield x, (-1, 1)
            return
        pipe = None
        if size:
            from .input_pipeline import GPUInputPipeline
            pipe = GPUInputPipeline(size, train=False)
        for batch, sizes in read_batches(files, batch_size, dec, device):
            if pipe is not None:
                yield pipe(batch.contiguous(), sizes), (-1, 1)
            else:
                same_size(sizes, "(", "): give --size")
                yield batch.permute(0, 3, 1, 2), "uint8"


def pair_slices(pairs, batch_size):
    """[(size, [(path_a, path_b)])]: the pairs grouped by Pillow's ``.size`` (w, h), the groups in sorted order, each cut into slices of
    ``batch_size``.  Only the headers are read.  A pair of unequal size is a ValueError that names both files."""
    from PIL import Image
    groups = {}
    for pa, pb in pairs:
        with Image.open(pa) as ia, Image.open(pb) as ib:
            if ia.size != ib.size:
                raise ValueError(f"{pa} is {ia.size[0]} x {ia.size[1]} but {pb} is {ib.size[0]} x {ib.size[1]}")
            groups.setdefault(ia.size, []).append((pa, pb))
    return [(size, groups[size][i:i + batch_size]) for size in sorted(groups) for i in range(0, len(groups[size]), batch_size)]


def paired_batches(dir_a, dir_b, batch_size, device):
    """Generator of (xa, xb) over the files of two directories paired by stem (``pair_files``), batched by size (``pair_slices``): uint8
    NCHW views of NHWC storage on ``device``, read through their strides."""
    for _, part in pair_slices(pair_files(dir_a, dir_b), batch_size):
        xa, xb = (padded_batch([read_rgb(p[k]) for p in part], device)[0].permute(0, 3, 1, 2) for k in (0, 1))
        yield xa, xb
