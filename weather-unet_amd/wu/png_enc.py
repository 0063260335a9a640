"""PNG encoding behind the inference and evaluation drivers (csrc/png_enc.hip): the lossless counterpart of ``wu.jpeg_enc``, for the
``.png`` variants of the reference's writers and for outputs that feed ``python -m wu.fid``, where JPEG artefacts bias the statistic.

Row filters (the minimum-sum-of-absolute-differences heuristic over the five PNG filters) and a literal-only dynamic-Huffman deflate
per 32 KiB segment of the filtered stream -- a stored block where that is not larger -- are parallel from end to end, so everything
runs on the GPU, checksums and framing included: three kernel launches per batch, and what crosses to the host is the finished files.
The files are 8-bit RGB, colour type 2, no interlace, no ancillary chunks.  They are NOT the bytes Pillow writes (Pillow runs zlib's
LZ77 matcher; these files are larger): they decode to the same pixels, and they equal ``tests/_png_enc_ref.encode`` byte for byte.
The output buffer is sized by the exact worst case (every segment stored), so there is no overflow and no Pillow fallback.

    enc = GPUPngEncoder()
    files = enc.encode_batch(images)                  # list[bytes]; images (N,H,W,3) uint8 or (N,3,H,W) fp32 / bf16 in [0, 1]
    enc.save_batch(images, paths)                     # the same bytes, written on the thread pool
    done = enc.save_batch_async(images, paths)        # ... without waiting: a Future; the next forward can be queued at once
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .jpeg import _Staging
from .jpeg_enc import _write
from .layout import stream_ptr

U8 = 2                                       # WU_PNG_ENC_U8
MAX_THREADS = 16


def segment_bytes():
    """Filtered bytes per deflate block.  Host only."""
    return int(_lib.load().wu_png_enc_segment_bytes())


def out_stride(h, w):
    """The exact worst case of an h x w file, every segment stored: the distance between two files in the output buffer.  Host only."""
    n = int(_lib.load().wu_png_enc_out_stride(int(h), int(w)))
    if n == 0:
        raise ValueError(f"png_enc: cannot encode {h} x {w}")
    return n


class _Plan:
    """What a batch geometry needs on the device besides the pixels: the descriptors (uploaded once, then reused -- also by a captured
    graph) and the sizes of the buffers every launch allocates."""
    def __init__(self, desc, ws_bytes, out_stride, n, hmax, wmax):
        self.desc, self.ws_bytes, self.out_stride = desc, ws_bytes, out_stride
        self.n, self.hmax, self.wmax = n, hmax, wmax


class DeviceResult:
    """Result of GPUPngEncoder.launch: the files on the device (image i at ``out[i * out_stride:]``) and their byte counts in
    ``result``."""
    def __init__(self, out, result, workspace, plan, images, sizes):
        self.out, self.result, self.workspace, self.plan = out, result, workspace, plan
        self.images, self.sizes = images, sizes
        self.n, self.out_stride = plan.n, plan.out_stride


class GPUPngEncoder:
    """Batch PNG encoder on the GPU.

    ``encode_batch(images, sizes)`` = ``fetch(launch(images, sizes))``.  ``launch`` runs the three kernels on the CURRENT stream and
    never synchronises; for a fixed batch geometry it can be captured in a ``torch.cuda.graph`` once one launch of that geometry has
    run outside the capture (that first launch uploads the descriptors).  ``fetch`` does one small device-to-host copy of the N byte
    counts, then one copy of exactly the used bytes into a pinned staging buffer.

    Staging-buffer rule (the decoder's): a buffer is refilled only after the event recorded behind the copy that wrote it has
    completed.

    ``images``: (N, H, W, 3) uint8, or (N, 3, H, W) float32 / bfloat16 with samples in [0, 1] (any strides: contiguous, channels-last,
    a slice ...), converted as ``wu.infer_driver.to_uint8`` does.  ``sizes``: [(h, w)] per image for a padded batch (what
    ``GPUJpegDecoder`` emits); the padding is never read.
    """
    def __init__(self, device="cuda", threads=None, max_staging=8):
        n = min(MAX_THREADS, os.cpu_count() or 1) if threads is None else int(threads)
        self.threads = max(1, min(MAX_THREADS, n))
        self.device = torch.device(device)
        self.max_staging = int(max_staging)
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="wu-png-enc")
        self._lock = threading.Lock()
        self._staging = []
        self._plans = {}
        self._io = self._side = None          # background writer of save_batch_async: one thread, one side stream, made on first use
        self.stats = {"native": 0, "bytes": 0}
        self._lib = _lib.load()
        assert self._lib.wu_png_enc_desc_bytes() == 16
        self.segment_bytes = int(self._lib.wu_png_enc_segment_bytes())

    def close(self):
        if self._io is not None:
            self._io.shutdown(wait=True)
        self._pool.shutdown(wait=True)

    # ---- staging buffers (the rule of GPUJpegDecoder._acquire) ----
    def _acquire(self, nbytes):
        with self._lock:
            free = [s for s in self._staging if not s.held]
            for s in free:
                if s.tensor.numel() >= nbytes and (s.event is None or s.event.query()):
                    s.held = True
                    return s
            if len(self._staging) >= self.max_staging and free:
                s = free[0]
                self._staging.remove(s)
                if s.event is not None:
                    s.event.synchronize()
            s = _Staging(max(int(nbytes * 1.25), 1 << 20), torch.cuda.is_available())
            s.held = True
            self._staging.append(s)
            return s

    def _release(self, s):
        with self._lock:
            s.held = False

    # ---- device stage ----
    @staticmethod
    def _geometry(images):
        """(dtype code, N, H, W, element strides (n, c, y, x))."""
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise ValueError("GPUPngEncoder: images must be a 4-d tensor, (N,H,W,3) uint8 or (N,3,H,W) float32 / bfloat16")
        if images.dtype == torch.uint8:
            if images.shape[3] != 3:
                raise ValueError(f"GPUPngEncoder: a uint8 batch is (N,H,W,3), got {tuple(images.shape)}")
            sn, sy, sx, sc = images.stride()
            return U8, images.shape[0], images.shape[1], images.shape[2], (sn, sc, sy, sx)
        if images.dtype in (torch.float32, torch.bfloat16):
            if images.shape[1] != 3:
                raise ValueError(f"GPUPngEncoder: a float batch is (N,3,H,W), got {tuple(images.shape)}")
            sn, sc, sy, sx = images.stride()
            return (_lib.F32 if images.dtype == torch.float32 else _lib.BF16), images.shape[0], images.shape[2], images.shape[3], (sn, sc, sy, sx)
        raise ValueError(f"GPUPngEncoder: dtype {images.dtype} is not uint8 / float32 / bfloat16")

    def _plan(self, n, hmax, wmax, sizes):
        key = (n, hmax, wmax, tuple(sizes))
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GPUPngEncoder.launch: this batch geometry has not been launched yet -- run launch once outside the "
                               "capture (it uploads the descriptors), then capture")
        ws_bytes = int(self._lib.wu_png_enc_workspace_bytes(n, hmax, wmax))
        stride = int(self._lib.wu_png_enc_out_stride(hmax, wmax))
        if ws_bytes == 0 or stride == 0:
            raise ValueError(f"GPUPngEncoder: cannot encode a batch of {n} images of up to {hmax} x {wmax}")
        desc = np.zeros((n, 4), dtype=np.int32)
        desc[:, :2] = sizes
        plan = _Plan(torch.from_numpy(desc).to(self.device), ws_bytes, stride, n, hmax, wmax)
        if len(self._plans) >= 64:                                    # a stream of ever-changing geometries must not grow without bound
            self._plans.pop(next(iter(self._plans)))
        self._plans[key] = plan
        return plan

    def launch(self, images, sizes=None):
        """The three kernels on the current stream; returns a DeviceResult."""
        dt, n, hmax, wmax, strides = self._geometry(images)
        if not images.is_cuda or not torch.cuda.is_available() or self.device.type != "cuda":
            raise RuntimeError("GPUPngEncoder: the encoder runs HIP kernels on an MI355X only -- there is no CPU fallback "
                               "(wu.png_enc.out_stride / segment_bytes are the host-only entry points)")
        if n < 1 or hmax < 1 or wmax < 1:
            raise ValueError("GPUPngEncoder: empty batch")
        if sizes is None:
            sizes = [(hmax, wmax)] * n
        sizes = [(int(h), int(w)) for h, w in sizes]
        if len(sizes) != n or any(not (1 <= h <= hmax and 1 <= w <= wmax) for h, w in sizes):
            raise ValueError(f"GPUPngEncoder: sizes must be {n} pairs (h, w) inside the batch's {hmax} x {wmax}")
        if any(s < 0 for s in strides):
            raise ValueError("GPUPngEncoder: negative strides")
        with torch.cuda.device(images.device):
            plan = self._plan(n, hmax, wmax, sizes)
            ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=images.device)
            out = torch.empty(n * plan.out_stride, dtype=torch.uint8, device=images.device)
            result = torch.empty(n, dtype=torch.int32, device=images.device)
            _lib.call("wu_png_enc_encode", images.data_ptr(), dt, strides[0], strides[1], strides[2], strides[3], plan.desc.data_ptr(),
                      ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), result.data_ptr(), n, hmax, wmax, stream_ptr())
        return DeviceResult(out, result, ws, plan, images, sizes)

    # ---- host stage ----
    def fetch(self, res):
        """list[bytes]: one complete PNG file per image of a launched batch."""
        with torch.cuda.device(res.out.device):
            counts = [int(c) for c in res.result.cpu().numpy()]          # the small copy: N byte counts
            if any(not 0 < c <= res.out_stride for c in counts):
                raise RuntimeError(f"GPUPngEncoder: byte counts {counts} outside (0, {res.out_stride}]")
            used = sum(counts)
            st = self._acquire(used)
            try:
                parts = [res.out[i * res.out_stride:i * res.out_stride + c] for i, c in enumerate(counts)]
                packed = parts[0] if len(parts) == 1 else torch.cat(parts)
                st.tensor[:used].copy_(packed, non_blocking=True)        # exactly the used bytes
                ev = torch.cuda.Event()
                ev.record()
                st.event = ev
                ev.synchronize()
                files, at = [], 0
                for c in counts:
                    files.append(st.array[at:at + c].tobytes())
                    at += c
            finally:
                self._release(st)
        with self._lock:
            self.stats["native"] += res.n
            self.stats["bytes"] += used
        return files

    def encode_batch(self, images, sizes=None):
        return self.fetch(self.launch(images, sizes))

    def save_batch(self, images, paths, sizes=None):
        """Encode and write ``paths[i]``; returns the byte counts."""
        paths = self._check_paths(images, paths)
        files = self.encode_batch(images, sizes)
        list(self._pool.map(_write, zip(paths, files)))
        return [len(f) for f in files]

    def save_batch_async(self, images, paths, sizes=None):
        """``save_batch`` without waiting: the kernels are launched on the current stream now, the copies to the host and the file
        writes happen on a background thread (on a side stream, behind an event recorded after the kernels), so the caller can
        queue the next forward at once.  Returns a Future of the byte counts; batches complete in the order they were submitted.
        The caller must not overwrite ``images`` before the Future is done."""
        paths = self._check_paths(images, paths)
        res = self.launch(images, sizes)
        with torch.cuda.device(res.out.device):
            ev = torch.cuda.Event()
            ev.record()
        with self._lock:
            if self._io is None:
                self._io = ThreadPoolExecutor(max_workers=1, thread_name_prefix="wu-png-enc-io")
                self._side = torch.cuda.Stream(device=res.out.device)
        return self._io.submit(self._finish_save, res, ev, paths)

    def _finish_save(self, res, ev, paths):
        with torch.cuda.device(res.out.device), torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            files = self.fetch(res)
        list(self._pool.map(_write, zip(paths, files)))
        return [len(f) for f in files]

    @staticmethod
    def _check_paths(images, paths):
        paths = [os.fspath(p) for p in paths]
        if len(paths) != images.shape[0]:
            raise ValueError(f"GPUPngEncoder: {len(paths)} paths for {images.shape[0]} images")
        return paths
