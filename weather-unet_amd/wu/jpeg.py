"""JPEG decoding in front of the GPU input pipeline (csrc/jpeg.hip): replaces ``Image.open(path).convert('RGB')`` of the reference's
loaders (dataset.py:64-67, 92-96, 128-129, 148-149).

The sequential part of JPEG (markers, Huffman codes) runs on host threads inside libwu_kernels.so -- ctypes releases the GIL around
the calls, so a thread pool scales; the data-parallel part (dequantisation, inverse DCT, chroma upsampling, YCbCr -> RGB, padding)
is two HIP kernel launches per batch that write the padded ``(N, Hmax, Wmax, 3)`` uint8 tensor ``GPUInputPipeline`` consumes.
The bytes equal Pillow's.  What the native path does not cover (progressive, CMYK, PNG, ...) is decoded by Pillow per image, on the
same worker thread, counted in ``stats`` and copied into its slot: the batch is always what the reference's loader saw.

    dec = GPUJpegDecoder()
    src_u8, sizes = dec.decode_batch(paths_or_bytes)
    images = GPUInputPipeline(224, ...)(src_u8, sizes)

``parse`` and ``entropy_decode`` are host-only and work without a GPU.
"""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _codec, _lib
from ._codec import MAX_THREADS  # noqa: F401 -- a public name of this module
from .layout import stream_ptr

MODE_GREY, MODE_444, MODE_H2V1, MODE_H2V2 = 0, 1, 2, 3
REASONS = {0: "ok", 1: "not-jpeg", 2: "corrupt-header", 3: "progressive", 4: "arithmetic", 5: "precision", 6: "lossless",
           7: "colorspace", 8: "qtable16", 9: "sampling", 10: "multiscan", 11: "magnitude"}
TILE_BLOCKS = 32          # blocks per IDCT workgroup (csrc/jpeg.hip kTileBlocks)
MAX_NATIVE_PIXELS = 89478485          # Pillow's Image.MAX_IMAGE_PIXELS default: larger images go through Pillow (which warns or refuses)


class JpegInfo(ctypes.Structure):
    """wu_jpeg_info of include/wu_kernels.h."""
    _fields_ = [("coef_bytes", ctypes.c_longlong), ("height", ctypes.c_int), ("width", ctypes.c_int), ("ncomp", ctypes.c_int),
                ("mode", ctypes.c_int), ("hs", ctypes.c_int * 3), ("vs", ctypes.c_int * 3), ("tq", ctypes.c_int * 3),
                ("td", ctypes.c_int * 3), ("ta", ctypes.c_int * 3), ("restart_interval", ctypes.c_int), ("mcus_x", ctypes.c_int),
                ("mcus_y", ctypes.c_int), ("blocks_w", ctypes.c_int * 3), ("blocks_h", ctypes.c_int * 3), ("total_blocks", ctypes.c_int),
                ("supported", ctypes.c_int), ("reason", ctypes.c_int), ("scan_offset", ctypes.c_int), ("dht_off", ctypes.c_int * 8),
                ("dqt_off", ctypes.c_int * 4), ("max_block_l1", ctypes.c_int), ("reserved", ctypes.c_int)]

    @property
    def reason_name(self):
        return REASONS.get(self.reason, str(self.reason))

    @property
    def sampling(self):
        """[(h, v)] per component."""
        return [(self.hs[c], self.vs[c]) for c in range(min(self.ncomp, 3))]


class JpegUnsupported(ValueError):
    """The file is not one the native path decodes; ``reason`` is one of REASONS' names."""
    def __init__(self, reason, what=""):
        super().__init__(f"jpeg: not decoded natively ({reason}){': ' + what if what else ''}")
        self.reason = reason


class JpegError(ValueError):
    """Corrupt entropy-coded data (bad Huffman code, bad restart sequence, premature end ...)."""


def _parse_bytes(lib, data):
    info = JpegInfo()
    _lib.check(lib.wu_jpeg_parse(data, len(data), ctypes.byref(info)), "wu_jpeg_parse")
    return info


def parse(data):
    """Header of a JPEG (bytes or path): a JpegInfo with height, width, sampling, restart_interval, supported, reason_name ...
    Host only."""
    lib = _lib.load()
    assert lib.wu_jpeg_info_bytes() == ctypes.sizeof(JpegInfo)
    return _parse_bytes(lib, _codec.read(data))


def _entropy_into(lib, data, info, coef_ptr, capacity, qtab_ptr):
    """0 = decoded, 1 = over the magnitude bound; raises JpegError on corrupt data."""
    rc = lib.wu_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef_ptr, capacity, qtab_ptr)
    if rc < 0:
        msg = lib.wu_last_error()
        raise JpegError(msg.decode() if msg else f"wu_jpeg_entropy_decode failed ({rc})")
    return rc


def entropy_decode(data):
    """Host stage alone (tests, tools): returns (planes, qtabs, info) with planes[c] a (blocks_h, blocks_w, 64) int16 array of
    QUANTISED coefficients in natural order and qtabs a (3, 64) uint16 array in natural order.  Raises JpegUnsupported / JpegError."""
    lib = _lib.load()
    data = _codec.read(data)
    info = _parse_bytes(lib, data)
    if not info.supported:
        raise JpegUnsupported(info.reason_name)
    coef = np.empty(info.total_blocks * 64, dtype=np.int16)
    qtabs = np.empty((3, 64), dtype=np.uint16)
    if _entropy_into(lib, data, info, coef.ctypes.data, coef.nbytes, qtabs.ctypes.data) == 1:
        raise JpegUnsupported("magnitude", f"max block L1 {info.max_block_l1}")
    planes, at = [], 0
    for c in range(info.ncomp):
        nb = info.blocks_h[c] * info.blocks_w[c]
        planes.append(coef[at * 64:(at + nb) * 64].reshape(info.blocks_h[c], info.blocks_w[c], 64))
        at += nb
    return planes, qtabs, info


class HostBatch(_codec.HostBatch):
    """Result of GPUJpegDecoder.prepare: entropy-decoded coefficients and descriptors of one batch in a staging buffer.  It owns
    the buffer until it is released (``release()`` or garbage collection), so it may be finished more than once."""
    def __init__(self, pool):
        super().__init__(pool)
        self.n = 0
        self.sizes = []
        self.hmax = self.wmax = 0
        self.n_tiles = 0
        self.off = {}
        self.fallbacks = []       # (slot, (h, w, 3) uint8 array) decoded by Pillow
        self.names = []


class DeviceBatch:
    """The uploaded coefficients, tables and descriptors of one batch plus the plane workspace: the arguments of wu_jpeg_reconstruct."""
    def __init__(self, buf, off, workspace, n, hmax, wmax, n_tiles):
        self.buf, self.off, self.workspace = buf, off, workspace
        self.n, self.hmax, self.wmax, self.n_tiles = n, hmax, wmax, n_tiles


class GPUJpegDecoder:
    """Batch JPEG decoder: host entropy stage on a thread pool, reconstruction on the GPU.

    ``decode_batch(items)`` = ``finish(prepare(items))``.  ``prepare`` reads, parses and Huffman-decodes on the pool into ONE staging
    buffer; it launches nothing and touches no stream, so a background thread may run it.  ``finish`` issues one non-blocking
    host-to-device copy of the used part of that buffer and the two reconstruction launches on the CURRENT stream, and belongs to
    the thread that owns the stream.

    Staging-buffer rule (``wu._codec.StagingPool``): a buffer may be refilled only after the copy that read it has completed.
    Every buffer carries an event recorded right after its copy; ``prepare`` takes a buffer only if no HostBatch holds it and its
    event has completed (checked with ``query()`` on the host, never waited for on the GPU), and allocates another one otherwise.
    Past ``max_staging`` buffers it blocks the HOST on the oldest event instead of growing further.
    """
    def __init__(self, device="cuda", threads=None, max_staging=8):
        self.threads = _codec.worker_threads(threads)
        self.device = torch.device(device)
        self.max_staging = int(max_staging)
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="wu-jpeg")
        self._lock = threading.Lock()
        self._staging = _codec.StagingPool(self.max_staging)
        self.stats = {"native": 0, "fallback": 0, "fallback_reasons": {}}
        self._lib = _lib.load()
        assert self._lib.wu_jpeg_info_bytes() == ctypes.sizeof(JpegInfo) and self._lib.wu_jpeg_desc_bytes() == 64

    def close(self):
        self._pool.shutdown(wait=True)

    # ---- host stage ----
    def _open(self, arg):
        i, item = arg
        data = _codec.read(item)
        info = _parse_bytes(self._lib, data)
        if info.supported and info.height * info.width <= MAX_NATIVE_PIXELS:
            return data, info, None, None
        # a header may claim any size up to 65535 x 65535: beyond Pillow's own decompression-bomb threshold the file is Pillow's to judge
        return data, info, _codec.pillow_rgb(data, _codec.name(item, i)), (info.reason_name if not info.supported else "too-large")

    def prepare(self, items):
        """Read + parse + entropy-decode ``items`` (bytes objects or paths) into a staging buffer; returns a HostBatch."""
        items = list(items)
        if not items:
            raise ValueError("GPUJpegDecoder: empty batch")
        opened = list(self._pool.map(self._open, enumerate(items)))
        hb = HostBatch(self._staging)
        hb.n = n = len(items)
        hb.names = [_codec.name(it, i) for i, it in enumerate(items)]
        first_block, first_tile, tiles = [0] * n, [0] * n, 0
        for i, (_, info, rgb, _) in enumerate(opened):
            first_tile[i], first_block[i] = tiles, tiles * TILE_BLOCKS
            if rgb is None:
                tiles += (info.total_blocks + TILE_BLOCKS - 1) // TILE_BLOCKS
        off = {"coef": 0}
        off["qtab"] = _codec.align(tiles * TILE_BLOCKS * 128)
        off["desc"] = _codec.align(off["qtab"] + n * 384)
        off["tile"] = _codec.align(off["desc"] + n * 64)
        hb.used = _codec.align(off["tile"] + max(tiles, 1) * 4)
        hb.off, hb.n_tiles = off, tiles
        st = hb.staging = self._staging.acquire(hb.used)
        desc = st.array[off["desc"]:off["desc"] + n * 64].view(np.int32).reshape(n, 16)
        tile = st.array[off["tile"]:off["tile"] + max(tiles, 1) * 4].view(np.int32)
        desc[:] = 0
        tile[:] = 0

        def decode(i):
            data, info, rgb, reason = opened[i]
            if rgb is not None:
                return rgb, reason
            cap = ((info.total_blocks + TILE_BLOCKS - 1) // TILE_BLOCKS) * TILE_BLOCKS * 128
            try:
                rc = _entropy_into(self._lib, data, info, st.ptr + first_block[i] * 128, cap, st.ptr + off["qtab"] + i * 384)
            except JpegError:
                return _codec.pillow_rgb(data, hb.names[i]), "corrupt-scan"      # Pillow is the arbiter; it raises on a truncated file
            if rc == 1:
                return _codec.pillow_rgb(data, hb.names[i]), "magnitude"
            return None, None

        results = list(self._pool.map(decode, range(n)))
        for i, ((_, info, _, _), (rgb, reason)) in enumerate(zip(opened, results)):
            _codec.count(self.stats, self._lock, reason)
            if rgb is not None:
                hb.fallbacks.append((i, rgb))
                hb.sizes.append((int(rgb.shape[0]), int(rgb.shape[1])))
                desc[i, 0], desc[i, 8] = first_block[i], first_tile[i]     # h = w = nblocks = 0: the kernels zero the whole slot
                continue
            hb.sizes.append((info.height, info.width))
            nt = (info.total_blocks + TILE_BLOCKS - 1) // TILE_BLOCKS
            bw_c, bh_c = (info.blocks_w[1], info.blocks_h[1]) if info.ncomp == 3 else (0, 0)
            desc[i, :10] = (first_block[i], info.height, info.width, info.mode, info.blocks_w[0], info.blocks_h[0], bw_c, bh_c,
                            first_tile[i], info.total_blocks)
            tile[first_tile[i]:first_tile[i] + nt] = i
        hb.hmax, hb.wmax = max(h for h, _ in hb.sizes), max(w for _, w in hb.sizes)
        return hb

    # ---- device stage ----
    def upload(self, hb):
        """One non-blocking H2D copy of the used part of the staging buffer (the event guarding the buffer is recorded after it)."""
        if not torch.cuda.is_available() or self.device.type != "cuda":
            raise RuntimeError("GPUJpegDecoder: the reconstruction runs HIP kernels on an MI355X only -- there is no CPU fallback "
                               "(wu.jpeg.parse / entropy_decode are the host-only entry points)")
        with torch.cuda.device(self.device):                          # the copy and its event go to this device's current stream
            buf = _codec.upload(hb, self.device, "GPUJpegDecoder")
            ws = torch.empty(max(int(self._lib.wu_jpeg_workspace_bytes(hb.n_tiles * TILE_BLOCKS)), 256), dtype=torch.uint8, device=self.device)
        return DeviceBatch(buf, hb.off, ws, hb.n, hb.hmax, hb.wmax, hb.n_tiles)

    def reconstruct(self, db, out=None):
        """wu_jpeg_reconstruct on the current stream; ``out``: an (N, Hmax, Wmax, 3) uint8 CUDA tensor to fill (allocated if None)."""
        if out is None:
            out = torch.empty((db.n, db.hmax, db.wmax, 3), dtype=torch.uint8, device=db.buf.device)
        if tuple(out.shape) != (db.n, db.hmax, db.wmax, 3) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("GPUJpegDecoder.reconstruct: out must be a contiguous (N, Hmax, Wmax, 3) uint8 CUDA tensor")
        base = db.buf.data_ptr()
        with torch.cuda.device(db.buf.device):
            _lib.call("wu_jpeg_reconstruct", base + db.off["coef"], base + db.off["desc"], base + db.off["tile"], base + db.off["qtab"],
                      db.workspace.data_ptr(), db.workspace.numel(), out.data_ptr(), db.n, db.hmax, db.wmax, db.n_tiles, stream_ptr())
        return out

    def finish(self, hb):
        """Upload + reconstruct + the Pillow-decoded slots; returns (src_u8 (N, Hmax, Wmax, 3) uint8 CUDA, [(h, w)] * N)."""
        db = self.upload(hb)
        out = self.reconstruct(db)
        with torch.cuda.device(self.device):
            for slot, rgb in hb.fallbacks:                             # the second, small H2D path: after the kernels zeroed the slot
                out[slot, :rgb.shape[0], :rgb.shape[1]] = torch.from_numpy(rgb).to(self.device)
        return out, list(hb.sizes)

    def decode_batch(self, items):
        hb = self.prepare(items)
        try:
            return self.finish(hb)
        finally:
            hb.release()
