"""JPEG encoding behind the inference and evaluation drivers (csrc/jpeg_enc.hip): replaces the ``save_image(output, '....jpg',
normalize=True)`` that ends the reference's inference scripts (inf_transfer_c.py:119-120, inf_transfer_e.py:141-142,
inf_1year_signals.py:105) -- one Pillow ``Image.save(path)`` per output image with Pillow's defaults (quality 75, 4:2:0, the
standard Huffman tables).

Baseline encoding is parallel from end to end, so everything runs on the GPU -- colour conversion, chroma downsampling, forward DCT,
quantisation, Huffman coding, byte stuffing, framing: five kernel launches per batch -- and what crosses to the host is the finished
files (a few tenths of a byte per pixel), not 3 bytes per pixel.  The bytes equal Pillow's.  An image whose entropy-coded data does
not fit its capacity (default: its raw size) is never truncated: it is encoded by Pillow from its pixels on a pool thread and
counted in ``stats``, exactly as the decoder counts its fallbacks.

    enc = GPUJpegEncoder(quality=75, subsampling="4:2:0")
    files = enc.encode_batch(images)                  # list[bytes]; images (N,H,W,3) uint8 or (N,3,H,W) fp32 / bf16 in [0, 1]
    enc.save_batch(images, paths)                     # the same bytes, written on the thread pool
    done = enc.save_batch_async(images, paths)        # ... without waiting: a Future; the next forward can be queued at once

``header`` and ``quant_tables`` are host-only and work without a GPU.
"""
import ctypes
import io
import threading

import numpy as np
import torch

from . import _codec, _lib
from ._codec import MAX_THREADS, U8  # noqa: F401 -- public names of this module; U8 is WU_JPEG_ENC_U8
from .layout import stream_ptr

SUBSAMPLING = {"4:2:0": 0, "4:4:4": 1}       # WU_JPEG_ENC_420 / WU_JPEG_ENC_444
_PILLOW_SUBSAMPLING = {"4:2:0": 2, "4:4:4": 0}
MIN_CAPACITY = 1024                          # bytes; a few-pixel image may well take more than its raw size


def _subsampling(s):
    if s in (0, "4:4:4"):                    # Pillow's spelling: subsampling=0
        return "4:4:4"
    if s in (2, "4:2:0", None):
        return "4:2:0"
    raise ValueError(f"jpeg_enc: subsampling {s!r} is neither '4:2:0' nor '4:4:4'")


def header(h, w, quality=75, subsampling="4:2:0"):
    """Everything in front of the entropy-coded data of an h x w file: SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS.  Host only."""
    lib = _lib.load()
    buf = (ctypes.c_uint8 * int(lib.wu_jpeg_enc_header_bytes()))()
    n = lib.wu_jpeg_enc_header(int(h), int(w), int(quality), SUBSAMPLING[_subsampling(subsampling)], buf, len(buf))
    if n <= 0:
        msg = lib.wu_last_error()
        raise ValueError(msg.decode() if msg else f"wu_jpeg_enc_header failed ({n})")
    return bytes(buf[:n])


def quant_tables(quality=75):
    """(2, 64) uint16: the luma and chroma quantisation tables of ``quality`` in natural order.  Host only."""
    lib = _lib.load()
    out = np.empty((2, 64), dtype=np.uint16)
    if lib.wu_jpeg_enc_qtables(int(quality), out.ctypes.data) != 0:
        raise ValueError(lib.wu_last_error().decode())
    return out


def _pillow_encode(rgb, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=_PILLOW_SUBSAMPLING[subsampling])
    return buf.getvalue()


class _Plan:
    """What a batch geometry needs on the device besides the pixels: descriptors and headers (uploaded once, then reused -- also by
    a captured graph) and the sizes of the buffers every launch allocates."""
    def __init__(self, desc, hdr, hdr_stride, ws_bytes, out_stride, cap_max, n, hmax, wmax):
        self.desc, self.hdr, self.hdr_stride = desc, hdr, hdr_stride
        self.ws_bytes, self.out_stride, self.cap_max = ws_bytes, out_stride, cap_max
        self.n, self.hmax, self.wmax = n, hmax, wmax


class DeviceResult:
    """Result of GPUJpegEncoder.launch: the files on the device (image i at ``out[i * out_stride:]``) and (bytes, overflow) per image
    in ``result``; ``images`` keeps the pixels for an image that has to go through Pillow."""
    def __init__(self, out, result, workspace, plan, images, sizes):
        self.out, self.result, self.workspace, self.plan = out, result, workspace, plan
        self.images, self.sizes = images, sizes
        self.n, self.out_stride = plan.n, plan.out_stride


class GPUJpegEncoder(_codec.BatchFileEncoder):
    """Batch JPEG encoder on the GPU with Pillow's bytes.

    ``encode_batch(images, sizes)`` = ``fetch(launch(images, sizes))``.  ``launch`` runs the five kernels on the CURRENT stream and
    never synchronises; for a fixed batch geometry it can be captured in a ``torch.cuda.graph`` once one launch of that geometry has
    run outside the capture (that first launch uploads the descriptors and headers).  ``fetch`` does one small device-to-host copy
    of the N byte counts and flags, then one copy of exactly the used bytes into a pinned staging buffer.

    ``save_batch`` / ``save_batch_async`` / ``close``: ``wu._codec.BatchFileEncoder``.  Staging buffers: ``wu._codec.StagingPool``.

    ``images``: (N, H, W, 3) uint8, or (N, 3, H, W) float32 / bfloat16 with samples in [0, 1] (any strides: contiguous, channels-last,
    a slice ...), converted as ``wu.infer_driver.to_uint8`` does.  ``sizes``: [(h, w)] per image for a padded batch (what
    ``GPUJpegDecoder`` emits); the padding is never read.
    """
    def __init__(self, device="cuda", quality=75, subsampling="4:2:0", threads=None, max_staging=8):
        self.device = torch.device(device)
        self.quality = int(quality)
        if not 1 <= self.quality <= 100:
            raise ValueError(f"GPUJpegEncoder: quality {quality} outside 1..100")
        self.subsampling = _subsampling(subsampling)
        self.max_staging = int(max_staging)
        self._start_pool(threads, "wu-jpeg-enc", "GPUJpegEncoder")
        self._lock = threading.Lock()         # guards stats
        self._staging = _codec.StagingPool(self.max_staging)
        self._plans = _codec.PlanCache("GPUJpegEncoder", "the descriptors and headers")
        self._qtab = None
        self.stats = {"native": 0, "fallback": 0, "fallback_reasons": {}}
        self._lib = _lib.load()
        assert self._lib.wu_jpeg_enc_desc_bytes() == 16
        self.header_bytes = int(self._lib.wu_jpeg_enc_header_bytes())

    def header(self, h, w):
        return header(h, w, self.quality, self.subsampling)

    # ---- device stage ----
    def _plan(self, n, hmax, wmax, sizes, capacity):
        return self._plans.get((n, hmax, wmax, tuple(sizes), capacity), lambda: self._make_plan(n, hmax, wmax, sizes, capacity))

    def _make_plan(self, n, hmax, wmax, sizes, capacity):
        caps = [max(h * w * 3, MIN_CAPACITY) if capacity is None else int(capacity) for h, w in sizes]
        cap_max = max(caps)
        sub = SUBSAMPLING[self.subsampling]
        ws_bytes = int(self._lib.wu_jpeg_enc_workspace_bytes(n, hmax, wmax, sub, cap_max))
        out_stride = int(self._lib.wu_jpeg_enc_out_stride(cap_max))
        if ws_bytes == 0 or out_stride == 0 or min(caps) < 1:
            raise ValueError(f"GPUJpegEncoder: cannot encode a batch of {n} images of up to {hmax} x {wmax} with capacity {cap_max}")
        desc = np.zeros((n, 4), dtype=np.int32)
        hdr_stride = (self.header_bytes + 15) // 16 * 16
        hdr = np.zeros((n, hdr_stride), dtype=np.uint8)
        for i, ((h, w), cap) in enumerate(zip(sizes, caps)):
            desc[i, :3] = (h, w, cap)
            hdr[i, :self.header_bytes] = np.frombuffer(self.header(h, w), dtype=np.uint8)
        if self._qtab is None:
            self._qtab = torch.from_numpy(quant_tables(self.quality).view(np.int16)).to(self.device)
        return _Plan(torch.from_numpy(desc).to(self.device), torch.from_numpy(hdr).to(self.device), hdr_stride, ws_bytes, out_stride,
                     cap_max, n, hmax, wmax)

    def launch(self, images, sizes=None, capacity=None):
        """The five kernels on the current stream; returns a DeviceResult.  ``capacity``: bytes of entropy-coded data each image may
        take (default: its raw size h * w * 3, at least 1 KiB)."""
        dt, n, hmax, wmax, strides = _codec.batch_geometry(images, "GPUJpegEncoder")
        if not images.is_cuda or not torch.cuda.is_available() or self.device.type != "cuda":
            raise RuntimeError("GPUJpegEncoder: the encoder runs HIP kernels on an MI355X only -- there is no CPU fallback "
                               "(wu.jpeg_enc.header / quant_tables are the host-only entry points)")
        sizes = _codec.check_sizes(n, hmax, wmax, sizes, strides, "GPUJpegEncoder")
        with torch.cuda.device(images.device):
            plan = self._plan(n, hmax, wmax, sizes, None if capacity is None else int(capacity))
            ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=images.device)
            out = torch.empty(n * plan.out_stride, dtype=torch.uint8, device=images.device)
            result = torch.empty((n, 2), dtype=torch.int32, device=images.device)
            _lib.call("wu_jpeg_enc_encode", images.data_ptr(), dt, strides[0], strides[1], strides[2], strides[3], plan.desc.data_ptr(),
                      self._qtab.data_ptr(), plan.hdr.data_ptr(), plan.hdr_stride, ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                      result.data_ptr(), n, hmax, wmax, SUBSAMPLING[self.subsampling], plan.cap_max, stream_ptr())
        return DeviceResult(out, result, ws, plan, images, sizes)

    # ---- host stage ----
    def _fallback(self, res, i):
        h, w = res.sizes[i]
        img = res.images[i]
        if img.dtype == torch.uint8:
            rgb = img[:h, :w].contiguous().cpu().numpy()
        else:                                                            # wu.infer_driver.to_uint8
            rgb = img[:, :h, :w].mul(255).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
        return self._pool.submit(_pillow_encode, rgb, self.quality, self.subsampling)

    def fetch(self, res):
        """list[bytes]: one complete JPEG file per image of a launched batch."""
        with torch.cuda.device(res.out.device):
            info = res.result.cpu().numpy()                              # the small copy: N x (bytes, overflow)
            native = [i for i in range(res.n) if not info[i, 1]]
            pending = {i: self._fallback(res, i) for i in range(res.n) if info[i, 1]}
            files = [None] * res.n
            counts = [int(c) for c in info[:, 0]]
            for i, f in zip(native, _codec.fetch_packed(self._staging, res.out, res.out_stride, counts, native)):
                files[i] = f
        for i in range(res.n):
            _codec.count(self.stats, self._lock, "capacity" if i in pending else None)
            if i in pending:
                files[i] = pending[i].result()
        return files

    def encode_batch(self, images, sizes=None, capacity=None):
        return self.fetch(self.launch(images, sizes, capacity))
