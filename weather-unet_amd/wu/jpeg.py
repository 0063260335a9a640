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

``GPUJpegDecoder(entropy="device")`` moves the Huffman decoding to the GPU as well (csrc/jpeg_huff.hip): the host only copies the
entropy-coded bytes of every file into the staging buffer (``scan_stage``), the compressed scan goes over the link instead of two bytes
per sample of coefficients, and ``finish`` waits once per batch for the device's verdict on every image.  Opt-in; the default is "host".

``GPUJpegDecoder(coverage="extended")`` decodes progressive files (every scan run on the host threads, csrc/jpeg_host.h) and 4:4:0
sampling natively instead of handing them to Pillow.  Opt-in; with the default "baseline" they are refused and counted as before.

``parse``, ``entropy_decode`` and ``scan_stage`` are host-only and work without a GPU.
"""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _codec, _lib
from ._codec import MAX_THREADS  # noqa: F401 -- a public name of this module
from .layout import stream_ptr

MODE_GREY, MODE_444, MODE_H2V1, MODE_H2V2, MODE_H1V2 = 0, 1, 2, 3, 4
REASONS = {0: "ok", 1: "not-jpeg", 2: "corrupt-header", 3: "progressive", 4: "arithmetic", 5: "precision", 6: "lossless",
           7: "colorspace", 8: "qtable16", 9: "sampling", 10: "multiscan", 11: "magnitude", 12: "progressive-incomplete"}
ALLOW_PROGRESSIVE, ALLOW_H1V2 = 1, 2          # WU_JPEG_ALLOW_*: the flags of wu_jpeg_parse_ex
COVERAGE = {"baseline": 0, "extended": ALLOW_PROGRESSIVE | ALLOW_H1V2}
FRAME_SEQUENTIAL, FRAME_PROGRESSIVE = 0, 1    # WU_JPEG_FRAME_*: JpegInfo.reserved
HUFF_STATUS = {0: "ok", 11: "magnitude"}          # a device status word by name; every other value: "corrupt-scan"
DHT_BYTES = 6 * 272       # raw DHT records of one image (csrc/jpeg_huff.hip kDhtImage)
DEFAULT_SUBSEQ_BITS = 1024          # WU_JPEG_HUFF_DEFAULT_SUBSEQ_BITS: the lowest kernel time of 256 / 512 / 1024 / 2048 (profiles/jpeg_huff_bench.md)
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
    def progressive(self):
        return self.reserved == FRAME_PROGRESSIVE

    @property
    def sampling(self):
        """[(h, v)] per component."""
        return [(self.hs[c], self.vs[c]) for c in range(min(self.ncomp, 3))]


class JpegScan(ctypes.Structure):
    """wu_jpeg_scan of include/wu_kernels.h."""
    _fields_ = [("scan_bytes", ctypes.c_int), ("n_segments", ctypes.c_int), ("n_subseq", ctypes.c_int), ("reserved", ctypes.c_int)]


def huff_status_name(code):
    return HUFF_STATUS.get(int(code), "corrupt-scan")


class JpegUnsupported(ValueError):
    """The file is not one the native path decodes; ``reason`` is one of REASONS' names."""
    def __init__(self, reason, what=""):
        super().__init__(f"jpeg: not decoded natively ({reason}){': ' + what if what else ''}")
        self.reason = reason


class JpegError(ValueError):
    """Corrupt entropy-coded data (bad Huffman code, bad restart sequence, premature end ...)."""


def _coverage_flags(coverage, who):
    if coverage not in COVERAGE:
        raise ValueError(f"{who}: coverage must be 'baseline' or 'extended', got {coverage!r}")
    return COVERAGE[coverage]


def _parse_bytes(lib, data, flags=0):
    info = JpegInfo()
    if flags:
        _lib.check(lib.wu_jpeg_parse_ex(data, len(data), ctypes.byref(info), flags), "wu_jpeg_parse_ex")
    else:
        _lib.check(lib.wu_jpeg_parse(data, len(data), ctypes.byref(info)), "wu_jpeg_parse")
    return info


def parse(data, coverage="baseline"):
    """Header of a JPEG (bytes or path): a JpegInfo with height, width, sampling, restart_interval, supported, reason_name ...
    ``coverage="extended"``: progressive frames and 4:4:0 sampling are reported supported too.  Host only."""
    flags = _coverage_flags(coverage, "wu.jpeg.parse")
    lib = _lib.load()
    assert lib.wu_jpeg_info_bytes() == ctypes.sizeof(JpegInfo)
    return _parse_bytes(lib, _codec.read(data), flags)


def _entropy_into(lib, data, info, coef_ptr, capacity, qtab_ptr):
    """0 = decoded, 1 = refused with ``info.reason`` set (over the magnitude bound; an incomplete progressive file); raises JpegError
    on corrupt data."""
    rc = lib.wu_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef_ptr, capacity, qtab_ptr)
    if rc < 0:
        msg = lib.wu_last_error()
        raise JpegError(msg.decode() if msg else f"wu_jpeg_entropy_decode failed ({rc})")
    return rc


def entropy_decode(data, coverage="baseline"):
    """Host stage alone (tests, tools): returns (planes, qtabs, info) with planes[c] a (blocks_h, blocks_w, 64) int16 array of
    QUANTISED coefficients in natural order and qtabs a (3, 64) uint16 array in natural order.  With ``coverage="extended"`` every scan
    of a progressive file is run into those planes.  Raises JpegUnsupported / JpegError."""
    flags = _coverage_flags(coverage, "wu.jpeg.entropy_decode")
    lib = _lib.load()
    data = _codec.read(data)
    info = _parse_bytes(lib, data, flags)
    if not info.supported:
        raise JpegUnsupported(info.reason_name)
    coef = np.empty(info.total_blocks * 64, dtype=np.int16)
    qtabs = np.empty((3, 64), dtype=np.uint16)
    if _entropy_into(lib, data, info, coef.ctypes.data, coef.nbytes, qtabs.ctypes.data) == 1:
        raise JpegUnsupported(info.reason_name, f"max block L1 {info.max_block_l1}" if info.reason == 11 else "")
    planes, at = [], 0
    for c in range(info.ncomp):
        nb = info.blocks_h[c] * info.blocks_w[c]
        planes.append(coef[at * 64:(at + nb) * 64].reshape(info.blocks_h[c], info.blocks_w[c], 64))
        at += nb
    return planes, qtabs, info


def _stage_into(lib, data, info, subseq_bits, scan_ptr, scan_cap, seg_ptr, seg_cap, dht_ptr, qtab_ptr):
    """wu_jpeg_scan_stage into caller-owned memory; returns the JpegScan, raises JpegError on a refusal."""
    res = JpegScan()
    rc = lib.wu_jpeg_scan_stage(data, len(data), ctypes.byref(info), subseq_bits, scan_ptr, scan_cap, seg_ptr, seg_cap, dht_ptr, qtab_ptr,
                                ctypes.byref(res))
    if rc < 0:
        msg = lib.wu_last_error()
        raise JpegError(msg.decode() if msg else f"wu_jpeg_scan_stage failed ({rc})")
    return res


def scan_stage(data, subseq_bits=DEFAULT_SUBSEQ_BITS):
    """Host staging alone (tests, tools): what ``entropy="device"`` uploads for one file.  Returns a dict: ``scan`` (uint8 array: the
    entropy-coded bytes, stuffing removed, every restart interval padded to whole subsequences), ``segs`` ((n, 4) int32: first_subseq,
    bit_length, first_mcu, mcu_count), ``dht`` (1632 bytes), ``qtab`` ((3, 64) uint16, natural order), ``n_subseq``, ``bound`` (what
    wu_jpeg_scan_stage_bytes promised) and ``info``.  Raises JpegUnsupported / JpegError."""
    lib = _lib.load()
    data = _codec.read(data)
    info = _parse_bytes(lib, data)
    if not info.supported:
        raise JpegUnsupported(info.reason_name)
    bound = int(lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), len(data), int(subseq_bits)))
    nseg = int(lib.wu_jpeg_scan_segments(ctypes.byref(info)))
    if bound == 0 or nseg == 0:
        raise JpegUnsupported("too-large", f"no staging bound at subseq_bits={subseq_bits}")
    scan = np.zeros(bound, np.uint8)
    segs = np.zeros((nseg, 4), np.int32)
    dht = np.zeros(DHT_BYTES, np.uint8)
    qtab = np.zeros((3, 64), np.uint16)
    res = _stage_into(lib, data, info, int(subseq_bits), scan.ctypes.data, scan.nbytes, segs.ctypes.data, segs.nbytes, dht.ctypes.data,
                      qtab.ctypes.data)
    return dict(scan=scan[:res.scan_bytes], segs=segs, dht=dht, qtab=qtab, n_subseq=res.n_subseq, bound=bound, info=info)


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
        self.entropy = "host"
        self.datas = []           # device entropy: the file bytes of the images the device may yet reject (None: settled in prepare)
        self.counted = False      # ... and whether their verdicts are in the decoder's stats already
        self.last_status = []     # per image: "ok", or the reason it was decoded by Pillow


class DeviceBatch:
    """The uploaded coefficients, tables and descriptors of one batch plus the plane workspace: the arguments of wu_jpeg_reconstruct."""
    def __init__(self, buf, off, workspace, n, hmax, wmax, n_tiles, coef=None):
        self.buf, self.off, self.workspace = buf, off, workspace
        self.n, self.hmax, self.wmax, self.n_tiles = n, hmax, wmax, n_tiles
        self.coef = coef          # device entropy: the device-only coefficient buffer (host entropy: they are part of ``buf``)


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

    ``entropy="device"`` (default "host": the path above, untouched): ``prepare`` parses and copies every file's entropy-coded bytes,
    segment table and raw tables into the staging buffer ([scan bytes | segment tables | DHT | qtab | Huffman desc | desc | tile map]);
    ``finish`` uploads that, runs wu_jpeg_huff_decode (subsequences of ``subseq_bits`` bits) into a device-only coefficient buffer and
    wu_jpeg_reconstruct, then copies the N status words back and waits for them -- ONE host synchronisation per batch, the rule of
    ``wu.png.GPUPngDecoder.finish``: whether the device accepted an image is known only then.  An image it rejects is decoded by Pillow
    into its slot and counted in ``stats`` under the status name ("magnitude", "corrupt-scan").

    ``coverage="extended"`` (default "baseline": everything above, untouched): progressive files and 4:4:0 sampling are decoded natively
    too and count as ``native``.  The scans of a progressive file are run on the worker thread into the same coefficient blocks, so the
    device half is the same two launches.  A progressive file whose scans stop short of full precision ("progressive-incomplete") still
    goes to Pillow, which smooths such a file between blocks.  Host entropy only: with ``entropy="device"`` it is a ValueError.
    """
    def __init__(self, device="cuda", threads=None, max_staging=8, entropy="host", subseq_bits=None, coverage="baseline"):
        if entropy not in ("host", "device"):
            raise ValueError(f"GPUJpegDecoder: entropy must be 'host' or 'device', got {entropy!r}")
        self._flags = _coverage_flags(coverage, "GPUJpegDecoder")
        if self._flags and entropy == "device":
            raise ValueError("GPUJpegDecoder: coverage='extended' needs entropy='host' -- the device Huffman walk knows one interleaved "
                             "baseline scan")
        self.entropy, self.coverage = entropy, coverage
        self.subseq_bits = DEFAULT_SUBSEQ_BITS if subseq_bits is None else int(subseq_bits)
        if self.subseq_bits % 32 or not 64 <= self.subseq_bits <= 4096:
            raise ValueError(f"GPUJpegDecoder: subseq_bits must be a multiple of 32 in [64, 4096], got {subseq_bits}")
        self.threads = _codec.worker_threads(threads)
        self.device = torch.device(device)
        self.max_staging = int(max_staging)
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="wu-jpeg")
        self._lock = threading.Lock()
        self._staging = _codec.StagingPool(self.max_staging)
        self.stats = {"native": 0, "fallback": 0, "fallback_reasons": {}}
        self._lib = _lib.load()
        assert self._lib.wu_jpeg_info_bytes() == ctypes.sizeof(JpegInfo) and self._lib.wu_jpeg_desc_bytes() == 64
        assert self._lib.wu_jpeg_huff_desc_bytes() == 64

    def close(self):
        self._pool.shutdown(wait=True)

    # ---- host stage ----
    def _open(self, arg):
        i, item = arg
        data = _codec.read(item)
        info = _parse_bytes(self._lib, data, self._flags)
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
        if self.entropy == "device":
            return self._prepare_device(hb, opened)
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
            if rc == 1:                                               # "magnitude", or "progressive-incomplete" / "qtable16" of a progressive file
                return _codec.pillow_rgb(data, hb.names[i]), info.reason_name
            return None, None

        results = list(self._pool.map(decode, range(n)))
        for i, ((_, info, _, _), (rgb, reason)) in enumerate(zip(opened, results)):
            _codec.count(self.stats, self._lock, reason)
            hb.last_status.append(reason or "ok")
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

    def _prepare_device(self, hb, opened):
        """The device-entropy half of ``prepare``: stage the scans instead of decoding them."""
        n, S, lib = hb.n, self.subseq_bits, self._lib
        hb.entropy = "device"
        opened = list(opened)
        bound, nseg = [0] * n, [0] * n
        for i, (data, info, rgb, reason) in enumerate(opened):
            if rgb is None:
                bound[i] = int(lib.wu_jpeg_scan_stage_bytes(ctypes.byref(info), len(data), S))
                nseg[i] = int(lib.wu_jpeg_scan_segments(ctypes.byref(info)))
                if bound[i] == 0 or nseg[i] == 0:                      # a scan of more than 2^28 bytes
                    opened[i] = (data, info, _codec.pillow_rgb(data, hb.names[i]), "too-large")
        scan_off, first_seg, first_block, first_tile = [0] * n, [0] * n, [0] * n, [0] * n
        at = segs = tiles = 0
        for i, (_, info, rgb, _) in enumerate(opened):
            scan_off[i], first_seg[i], first_tile[i], first_block[i] = at, segs, tiles, tiles * TILE_BLOCKS
            if rgb is None:
                at += bound[i]                                         # a multiple of 16
                segs += nseg[i]
                tiles += (info.total_blocks + TILE_BLOCKS - 1) // TILE_BLOCKS
        off = {"scan": 0}
        off["seg"] = _codec.align(max(at, 16))
        off["dht"] = _codec.align(off["seg"] + max(segs, 1) * 16)
        off["qtab"] = _codec.align(off["dht"] + n * DHT_BYTES)
        off["hdesc"] = _codec.align(off["qtab"] + n * 384)
        off["desc"] = _codec.align(off["hdesc"] + n * 64)
        off["tile"] = _codec.align(off["desc"] + n * 64)
        hb.used = _codec.align(off["tile"] + max(tiles, 1) * 4)
        hb.off, hb.n_tiles = off, tiles
        st = hb.staging = self._staging.acquire(hb.used)
        hdesc = st.array[off["hdesc"]:off["hdesc"] + n * 64].view(np.int32).reshape(n, 16)
        desc = st.array[off["desc"]:off["desc"] + n * 64].view(np.int32).reshape(n, 16)
        tile = st.array[off["tile"]:off["tile"] + max(tiles, 1) * 4].view(np.int32)
        hdesc[:] = 0
        desc[:] = 0
        tile[:] = 0

        def stage(i):
            data, info, rgb, reason = opened[i]
            if rgb is not None:
                return rgb, reason, None
            try:
                res = _stage_into(lib, data, info, S, st.ptr + off["scan"] + scan_off[i], bound[i], st.ptr + off["seg"] + first_seg[i] * 16,
                                  nseg[i] * 16, st.ptr + off["dht"] + i * DHT_BYTES, st.ptr + off["qtab"] + i * 384)
            except JpegError:
                return _codec.pillow_rgb(data, hb.names[i]), "corrupt-scan", None      # Pillow is the arbiter; it raises on a truncated file
            return None, None, res

        results = list(self._pool.map(stage, range(n)))
        for i, ((data, info, _, _), (rgb, reason, res)) in enumerate(zip(opened, results)):
            if rgb is not None:
                _codec.count(self.stats, self._lock, reason)
                hb.last_status.append(reason)
                hb.datas.append(None)
                hb.fallbacks.append((i, rgb))
                hb.sizes.append((int(rgb.shape[0]), int(rgb.shape[1])))
                desc[i, 0], desc[i, 8] = first_block[i], first_tile[i]     # h = w = nblocks = 0, no subsequences: nothing is decoded
                hdesc[i, 5] = first_block[i]
                continue
            hb.last_status.append("ok")
            hb.datas.append(data)
            hb.sizes.append((info.height, info.width))
            nt = (info.total_blocks + TILE_BLOCKS - 1) // TILE_BLOCKS
            bw_c, bh_c = (info.blocks_w[1], info.blocks_h[1]) if info.ncomp == 3 else (0, 0)
            desc[i, :10] = (first_block[i], info.height, info.width, info.mode, info.blocks_w[0], info.blocks_h[0], bw_c, bh_c,
                            first_tile[i], info.total_blocks)
            hdesc[i, :13] = (scan_off[i], res.scan_bytes, first_seg[i], res.n_segments, res.n_subseq, first_block[i], info.total_blocks,
                             info.ncomp, info.hs[0], info.vs[0], info.mcus_x, info.mcus_x * info.mcus_y, info.restart_interval)
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
            coef = None
            if hb.entropy == "device":                                 # never uploaded: wu_jpeg_huff_decode fills it
                coef = torch.empty(max(hb.n_tiles * TILE_BLOCKS * 128, 256), dtype=torch.uint8, device=self.device)
        return DeviceBatch(buf, hb.off, ws, hb.n, hb.hmax, hb.wmax, hb.n_tiles, coef)

    def huff_decode(self, db):
        """wu_jpeg_huff_decode on the current stream (device entropy); returns the (N,) int32 CUDA tensor of status words."""
        if db.coef is None:
            raise ValueError("GPUJpegDecoder.huff_decode: this batch was prepared with entropy='host'")
        base = db.buf.data_ptr()
        with torch.cuda.device(db.buf.device):
            status = torch.empty(db.n, dtype=torch.int32, device=db.buf.device)
            _lib.call("wu_jpeg_huff_decode", base + db.off["scan"], base + db.off["seg"], base + db.off["dht"], base + db.off["hdesc"],
                      base + db.off["qtab"], db.coef.data_ptr(), status.data_ptr(), db.n, self.subseq_bits, stream_ptr())
        return status

    def reconstruct(self, db, out=None):
        """wu_jpeg_reconstruct on the current stream; ``out``: an (N, Hmax, Wmax, 3) uint8 CUDA tensor to fill (allocated if None)."""
        if out is None:
            out = torch.empty((db.n, db.hmax, db.wmax, 3), dtype=torch.uint8, device=db.buf.device)
        if tuple(out.shape) != (db.n, db.hmax, db.wmax, 3) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("GPUJpegDecoder.reconstruct: out must be a contiguous (N, Hmax, Wmax, 3) uint8 CUDA tensor")
        base = db.buf.data_ptr()
        coef_ptr = db.coef.data_ptr() if db.coef is not None else base + db.off["coef"]
        with torch.cuda.device(db.buf.device):
            _lib.call("wu_jpeg_reconstruct", coef_ptr, base + db.off["desc"], base + db.off["tile"], base + db.off["qtab"],
                      db.workspace.data_ptr(), db.workspace.numel(), out.data_ptr(), db.n, db.hmax, db.wmax, db.n_tiles, stream_ptr())
        return out

    def finish(self, hb):
        """Upload + reconstruct + the Pillow-decoded slots; returns (src_u8 (N, Hmax, Wmax, 3) uint8 CUDA, [(h, w)] * N)."""
        db = self.upload(hb)
        late = []
        if hb.entropy == "device":
            status = self.huff_decode(db)
            out = self.reconstruct(db)
            codes = status.cpu().numpy()                               # waits for the kernels: a rejection is known only now
            for i, code in enumerate(codes):
                if hb.datas[i] is None:
                    continue
                name = huff_status_name(code)
                if not hb.counted:
                    _codec.count(self.stats, self._lock, None if code == 0 else name)
                hb.last_status[i] = name
                if code == 0:
                    continue
                rgb = _codec.pillow_rgb(hb.datas[i], hb.names[i])          # Pillow is the arbiter; it raises on a truncated file
                if rgb.shape[:2] != hb.sizes[i]:
                    raise RuntimeError(f"cannot decode image {hb.names[i]}: Pillow reads {rgb.shape[1]} x {rgb.shape[0]}, the header "
                                       f"says {hb.sizes[i][1]} x {hb.sizes[i][0]}")
                late.append((i, rgb))
            hb.counted = True
        else:
            out = self.reconstruct(db)
        with torch.cuda.device(self.device):
            for slot, rgb in hb.fallbacks + late:                      # the second, small H2D path: over whatever the kernels left in the slot
                out[slot, :rgb.shape[0], :rgb.shape[1]] = torch.from_numpy(rgb).to(self.device)
        return out, list(hb.sizes)

    def decode_batch(self, items, return_status=False):
        """(src_u8, sizes), and with ``return_status`` a third item as in ``wu.png``: per image "ok", or the reason Pillow decoded it."""
        hb = self.prepare(items)
        try:
            out, sizes = self.finish(hb)
        finally:
            hb.release()
        if return_status:
            return out, sizes, list(hb.last_status)
        return out, sizes
