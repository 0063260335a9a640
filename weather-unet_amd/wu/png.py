"""PNG decoding in front of the FID and evaluation readers (csrc/png_dec.hip): the counterpart of ``wu.png_enc`` and the PNG sibling of
``wu.jpeg.GPUJpegDecoder``, with the same interface and the same padded ``(N, Hmax, Wmax, 3)`` uint8 result.

Taken natively: 8-bit RGB, non-interlaced files whose IDAT chunks are independent 32 KiB deflate segments -- what ``GPUPngEncoder``
writes, and what zlib's ``Z_FULL_FLUSH`` every 32 KiB or ``pigz -i`` produce.  The host only walks the chunk headers
(``wu_png_dec_parse``, C inside the library, no GPU needed); the file bytes go up in one copy and two kernel launches inflate every
segment of the batch (full RFC 1951, one wave per segment), check the CRC-32 of every IDAT chunk and the Adler-32, and undo the row
filters.  Everything else -- grey, palette, alpha, 16-bit, interlaced, ordinary one-stream PNGs, JPEGs -- is decoded by Pillow per image,
counted in ``stats`` under the parser's reason; so is a file the device rejects (a corrupt one, or a foreign one with the right chunk
count by coincidence), counted under the device's status.  Pillow is the arbiter: if it raises, the error propagates with the file's name.

    dec = GPUPngDecoder()
    src_u8, sizes = dec.decode_batch(paths_or_bytes)
    src_u8, sizes, statuses = dec.decode_batch(paths_or_bytes, return_status=True)      # the device's verdict per image, by name
    src_u8, sizes = decode_mixed(paths_or_bytes)                                         # the same with a decoder made on the spot

Unlike the JPEG decoder, ``finish`` synchronises with the device once per batch: whether an image was accepted is known only after the
kernels ran, so the N status words are copied back and waited for before the rejected slots are filled.

``parse`` is host-only and works without a GPU; so do ``prepare`` and ``buffer_sizes``.
"""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _codec, _lib
from .jpeg import MAX_NATIVE_PIXELS
from .layout import stream_ptr

SIGNATURE = b"\x89PNG\r\n\x1a\n"
REASONS = {0: "ok", 1: "not-png", 2: "header", 3: "colour-type", 4: "bit-depth", 5: "interlaced", 6: "not-segmented", 7: "too-large",
           8: "corrupt-chunk"}
STATUS = {0: "ok", 1: "chunk-crc", 2: "bad-stream", 3: "distance", 4: "segment-size", 5: "filter-type", 6: "adler"}
DESC_BYTES, SEG_BYTES = 32, 16
DESC_DTYPE = np.dtype([("src_off", "<i8"), ("file_bytes", "<i4"), ("h", "<i4"), ("w", "<i4"), ("first_seg", "<i4"), ("nseg", "<i4"),
                       ("pad", "<i4")])
SEG_DTYPE = np.dtype([("image", "<i4"), ("k", "<i4"), ("off", "<u4"), ("len", "<u4")])


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
    return _parse_bytes(lib, _codec.read(data), max_pixels)


class HostBatch(_codec.HostBatch):
    """Result of GPUPngDecoder.prepare: the files of one batch, their descriptors and the segment table in a staging buffer.  It owns
    the buffer until it is released (``release()`` or garbage collection), so it may be finished more than once."""
    def __init__(self, pool):
        super().__init__(pool)
        self.n = 0
        self.sizes = []
        self.hmax = self.wmax = 0
        self.n_segments = 0
        self.off = {}
        self.file_off = []        # per image: offset of its bytes in the staging buffer (None: decoded by Pillow in prepare)
        self.file_len = []
        self.datas = []           # the files' bytes, for the images the device may yet reject
        self.fallbacks = []       # (slot, (h, w, 3) uint8 array) decoded by Pillow in prepare
        self.names = []
        self.counted = False      # its images are in the decoder's stats
        self.last_status = None   # device status per image of the last finish


class GPUPngDecoder:
    """Batch PNG decoder: chunk headers on a thread pool, inflate and unfilter on the GPU.

    ``decode_batch(items)`` = ``finish(prepare(items))``.  ``prepare`` reads and parses on the pool, copies the native files' bytes
    into ONE staging buffer and decodes the files the parser refuses with Pillow; it launches nothing and touches no stream, so a
    background thread may run it.  ``finish`` issues one non-blocking host-to-device copy of the used part of that buffer and the two
    launches on the CURRENT stream, then copies the N status words back and waits for them -- one host synchronisation per batch --
    and decodes the images the device rejected with Pillow into their zeroed slots.

    Staging buffers: ``wu._codec.StagingPool``.

    ``stats``: images decoded natively, images decoded by Pillow, and the latter by reason (a parser reason or a device status).
    """
    def __init__(self, device="cuda", threads=None, max_staging=8):
        self.threads = _codec.worker_threads(threads)
        self.device = torch.device(device)
        self.max_staging = int(max_staging)
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="wu-png")
        self._lock = threading.Lock()
        self._staging = _codec.StagingPool(self.max_staging)
        self.stats = {"native": 0, "fallback": 0, "fallback_reasons": {}}
        self._lib = _lib.load()
        assert (self._lib.wu_png_dec_info_bytes() == ctypes.sizeof(PngInfo) and self._lib.wu_png_dec_desc_bytes() == DESC_BYTES
                == DESC_DTYPE.itemsize and self._lib.wu_png_dec_seg_bytes() == SEG_BYTES == SEG_DTYPE.itemsize)

    def close(self):
        self._pool.shutdown(wait=True)

    # ---- host stage ----
    def _open(self, arg):
        i, item = arg
        data = _codec.read(item)
        info, idat = _parse_bytes(self._lib, data)
        if info.supported and len(data) < 1 << 31:                     # the descriptors hold 32-bit offsets inside a file
            return data, info, idat, None, None
        return data, info, idat, _codec.pillow_rgb(data, _codec.name(item, i)), (info.reason_name if not info.supported else "too-large")

    def prepare(self, items):
        """Read + parse ``items`` (bytes objects or paths) and stage the native files; returns a HostBatch.  Needs no GPU."""
        items = list(items)
        if not items:
            raise ValueError("GPUPngDecoder: empty batch")
        opened = list(self._pool.map(self._open, enumerate(items)))
        hb = HostBatch(self._staging)
        hb.n = n = len(items)
        hb.names = [_codec.name(it, i) for i, it in enumerate(items)]
        at, segs = 0, 0
        first_seg = [0] * n
        for i, (data, info, idat, rgb, reason) in enumerate(opened):
            first_seg[i] = segs
            if rgb is None:
                hb.file_off.append(at)
                hb.file_len.append(len(data))
                hb.datas.append(data)
                hb.sizes.append((info.height, info.width))
                at = _codec.align(at + len(data), 16)
                segs += info.n_segments
            else:
                _codec.count(self.stats, self._lock, reason)
                hb.file_off.append(None)
                hb.file_len.append(0)
                hb.datas.append(None)
                hb.fallbacks.append((i, rgb))
                hb.sizes.append((int(rgb.shape[0]), int(rgb.shape[1])))
        off = {"files": 0}
        off["desc"] = _codec.align(at)
        off["seg"] = _codec.align(off["desc"] + n * DESC_BYTES)
        hb.used = _codec.align(off["seg"] + max(segs, 1) * SEG_BYTES)
        hb.off, hb.n_segments = off, segs
        st = hb.staging = self._staging.acquire(hb.used)
        desc = st.array[off["desc"]:off["desc"] + n * DESC_BYTES].view(DESC_DTYPE)
        seg = st.array[off["seg"]:off["seg"] + max(segs, 1) * SEG_BYTES].view(SEG_DTYPE)
        desc[:] = 0
        seg[:] = 0

        def stage(i):
            data, info, idat, rgb, _ = opened[i]
            if rgb is not None:
                return                                                 # h = w = 0: the kernels zero the whole slot
            a = hb.file_off[i]
            st.array[a:a + len(data)] = np.frombuffer(data, dtype=np.uint8)
            desc[i] = (a, len(data), info.height, info.width, first_seg[i], info.n_segments, 0)
            rows = seg[first_seg[i]:first_seg[i] + info.n_segments]
            rows["image"] = i
            rows["k"] = np.arange(info.n_segments)
            rows["off"] = idat[:, 0]
            rows["len"] = idat[:, 1]

        list(self._pool.map(stage, range(n)))
        hb.hmax, hb.wmax = max(h for h, _ in hb.sizes), max(w for _, w in hb.sizes)
        return hb

    def buffer_sizes(self, hb):
        """Bytes of every device buffer ``finish`` hands to wu_png_dec_decode for this batch; needs no GPU."""
        ws_bytes = int(self._lib.wu_png_dec_workspace_bytes(hb.n, hb.hmax, hb.wmax, hb.n_segments))
        if ws_bytes == 0:
            raise ValueError(f"GPUPngDecoder: cannot decode a batch of {hb.n} images of up to {hb.hmax} x {hb.wmax}")
        return {"source": hb.off["desc"], "desc": hb.n * DESC_BYTES, "seg": max(hb.n_segments, 1) * SEG_BYTES, "upload": hb.used,
                "workspace": ws_bytes, "out": hb.n * hb.hmax * hb.wmax * 3, "status": hb.n * 4}

    # ---- device stage ----
    def finish(self, hb):
        """Upload + inflate + unfilter, the status words back (the one synchronisation), Pillow for what was refused or rejected;
        returns (src_u8 (N, Hmax, Wmax, 3) uint8 CUDA, [(h, w)] * N)."""
        if not torch.cuda.is_available() or self.device.type != "cuda":
            raise RuntimeError("GPUPngDecoder: inflate and unfilter run HIP kernels on an MI355X only -- there is no CPU fallback "
                               "(wu.png.parse is the host-only entry point)")
        if hb.staging is None:                                        # before anything else about the batch is judged
            raise RuntimeError("GPUPngDecoder: this HostBatch was released")
        sizes = self.buffer_sizes(hb)
        ws_bytes = sizes["workspace"]
        with torch.cuda.device(self.device):                          # the copy and its event go to this device's current stream
            buf = _codec.upload(hb, self.device, "GPUPngDecoder")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            out = torch.empty((hb.n, hb.hmax, hb.wmax, 3), dtype=torch.uint8, device=self.device)
            status = torch.empty(hb.n, dtype=torch.int32, device=self.device)
            base = buf.data_ptr()
            _lib.call("wu_png_dec_decode", base, hb.off["desc"], base + hb.off["desc"], hb.n * DESC_BYTES, base + hb.off["seg"],
                      max(hb.n_segments, 1) * SEG_BYTES, hb.n_segments, ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                      status.data_ptr(), status.numel() * 4, hb.n, hb.hmax, hb.wmax, stream_ptr())
            codes = status.cpu().numpy()                               # waits for the kernels: a rejection is known only now
            late = []
            for i, code in enumerate(codes):
                if hb.datas[i] is None:
                    continue
                if code == 0:
                    if not hb.counted:
                        _codec.count(self.stats, self._lock, None)
                    continue
                rgb = _codec.pillow_rgb(hb.datas[i], hb.names[i])
                if rgb.shape[:2] != hb.sizes[i]:
                    raise RuntimeError(f"cannot decode image {hb.names[i]}: Pillow reads {rgb.shape[1]} x {rgb.shape[0]}, the header "
                                       f"says {hb.sizes[i][1]} x {hb.sizes[i][0]}")
                if not hb.counted:
                    _codec.count(self.stats, self._lock, STATUS.get(int(code), str(int(code))))
                late.append((i, rgb))
            hb.counted = True
            for slot, rgb in hb.fallbacks + late:                      # the second, small H2D path: the kernels zeroed these slots
                out[slot, :rgb.shape[0], :rgb.shape[1]] = torch.from_numpy(rgb).to(self.device)
        hb.last_status = [int(c) for c in codes]
        return out, list(hb.sizes)

    def decode_batch(self, items, return_status=False):
        """(src_u8, sizes), and with ``return_status`` the device's verdict per image as a third item: a name of STATUS, "ok" too for an
        image the parser sent to Pillow."""
        hb = self.prepare(items)
        try:
            out, sizes = self.finish(hb)
        finally:
            hb.release()
        if return_status:
            return out, sizes, [STATUS.get(c, str(c)) for c in hb.last_status]
        return out, sizes


def decode_mixed(files, decoder=None):
    """One batch of image files (paths or bytes) in the given order: segmented 8-bit RGB PNGs are decoded on the GPU, files the parser
    refuses (any other PNG, a JPEG) and files the device rejects by Pillow.  Returns ((N, Hmax, Wmax, 3) uint8 CUDA tensor, [(h, w)]);
    ``decoder``: a GPUPngDecoder to use (and to read ``stats`` from) instead of one made and closed here."""
    if decoder is not None:
        return decoder.decode_batch(files)
    dec = GPUPngDecoder()
    try:
        return dec.decode_batch(files)
    finally:
        dec.close()
