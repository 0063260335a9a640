"""PNG files whose IDAT chunks are independent 32 KiB deflate segments (csrc/png_dec.hip): the host-side header parse.

``wu.png_enc.GPUPngEncoder`` writes such files, and so do zlib's ``Z_FULL_FLUSH`` every 32 KiB and ``pigz -i``: 8-bit RGB, non-interlaced,
IDAT chunk k holding the deflate data of bytes [32768 k, 32768 (k + 1)) of the filtered stream, so the segment boundaries are the chunk
boundaries and every segment can be inflated on its own.  ``parse`` walks the chunk headers (C inside the library, twelve bytes per chunk,
no GPU) and says whether a file is of that class -- with a reason when it is not -- and where its segments lie.  There is no device
stage yet: files are still decoded by Pillow (``wu.jpeg.GPUJpegDecoder`` counts them under ``not-jpeg``).

    info, idat = parse(path_or_bytes)        # info.supported, info.reason_name, info.height, info.width; idat: (n, 2) offsets and lengths
"""
import ctypes

import numpy as np

from . import _lib
from .jpeg import MAX_NATIVE_PIXELS, _read

REASONS = {0: "ok", 1: "not-png", 2: "header", 3: "colour-type", 4: "bit-depth", 5: "interlaced", 6: "not-segmented", 7: "too-large",
           8: "corrupt-chunk"}


class PngInfo(ctypes.Structure):
    """wu_png_dec_info of include/wu_kernels.h."""
    _fields_ = [("filtered_bytes", ctypes.c_longlong), ("height", ctypes.c_int), ("width", ctypes.c_int), ("bit_depth", ctypes.c_int),
                ("colour_type", ctypes.c_int), ("interlace", ctypes.c_int), ("n_idat", ctypes.c_int), ("n_segments", ctypes.c_int),
                ("supported", ctypes.c_int), ("reason", ctypes.c_int), ("reserved", ctypes.c_int)]

    @property
    def reason_name(self):
        return REASONS.get(self.reason, str(self.reason))


def _parse_bytes(lib, data, max_pixels=MAX_NATIVE_PIXELS):
    """(PngInfo, (n_idat, 2) int64 array of IDAT body offsets and lengths -- empty unless the file is supported)."""
    info = PngInfo()
    cap = 64
    while True:
        idat = np.empty((cap, 2), dtype=np.int64)
        _lib.check(lib.wu_png_dec_parse(data, len(data), int(max_pixels), ctypes.byref(info), idat.ctypes.data, cap), "wu_png_dec_parse")
        if not info.supported:
            return info, idat[:0]
        if info.n_idat <= cap:
            return info, idat[:info.n_idat]
        cap = info.n_idat


def parse(data, max_pixels=MAX_NATIVE_PIXELS):
    """Header of a PNG (bytes or path): (PngInfo with height, width, supported, reason_name ..., IDAT (offset, length) array).
    Host only."""
    lib = _lib.load()
    assert lib.wu_png_dec_info_bytes() == ctypes.sizeof(PngInfo)
    return _parse_bytes(lib, _read(data), max_pixels)
