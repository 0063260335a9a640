"""Host plumbing the image codecs share (wu.jpeg, wu.png, wu.jpeg_enc, wu.png_enc, wu.gif_enc): the staging-buffer pool, the batch
geometry of the encoders, the plan cache, the one device-to-host fetch of finished files, the file saving of the batch encoders and the
upload of the decoders.  What differs between the codecs stays in their own modules.
"""
import io
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

MAX_THREADS = 16
U8 = 2                                       # WU_JPEG_ENC_U8 == WU_PNG_ENC_U8: the uint8 sample code besides _lib.F32 / _lib.BF16


# ---- small helpers ----
def read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(os.fspath(item), "rb") as fh:
        return fh.read()


def write(arg):
    path, data = arg
    with open(path, "wb") as fh:
        fh.write(data)


def name(item, i=None):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return f"<bytes #{i}>" if i is not None else "<bytes>"
    return os.fspath(item)


def pillow_rgb(data, what):
    from PIL import Image
    try:
        return np.array(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)          # a writable, contiguous copy
    except Exception as e:                                              # noqa: BLE001 -- whatever Pillow raises, name the file
        raise RuntimeError(f"cannot decode image {what}: {type(e).__name__}: {e}") from e


def align(v, a=256):
    return (v + a - 1) // a * a


def worker_threads(threads):
    """Size of a codec's thread pool: ``threads``, or one per CPU, inside 1 .. MAX_THREADS."""
    n = min(MAX_THREADS, os.cpu_count() or 1) if threads is None else int(threads)
    return max(1, min(MAX_THREADS, n))


def count(stats, lock, reason):
    """One image into ``stats``: native if ``reason`` is None, else a fallback under that reason."""
    with lock:
        if reason is None:
            stats["native"] += 1
        else:
            stats["fallback"] += 1
            stats["fallback_reasons"][reason] = stats["fallback_reasons"].get(reason, 0) + 1


# ---- staging buffers ----
class Staging:
    """One host staging buffer (pinned when a GPU is present) and the event recorded after the last copy that used it."""
    def __init__(self, nbytes, pinned):
        self.tensor = torch.empty(nbytes, dtype=torch.uint8, pin_memory=pinned)
        self.array = self.tensor.numpy()
        self.ptr = self.tensor.data_ptr()
        self.event = None         # torch.cuda.Event of the last copy out of or into this buffer
        self.held = False         # a HostBatch or a fetch owns it


class StagingPool:
    """The staging-buffer rule: a buffer may be refilled only after the copy that used it has completed.  Every buffer carries the
    event recorded right after its copy; ``acquire`` hands out a buffer only if nobody holds it and its event has completed (checked
    with ``query()`` on the host, never waited for on the GPU), and allocates another one otherwise.  Past ``max_staging`` buffers it
    blocks the HOST on the oldest free buffer's event instead of growing further."""
    def __init__(self, max_staging):
        self.max_staging = int(max_staging)
        self._lock = threading.Lock()
        self._buffers = []

    def __len__(self):
        return len(self._buffers)

    def acquire(self, nbytes):
        with self._lock:
            free = [s for s in self._buffers if not s.held]
            for s in free:
                if s.tensor.numel() >= nbytes and (s.event is None or s.event.query()):
                    s.held = True
                    return s
            if len(self._buffers) >= self.max_staging and free:
                s = free[0]                                            # full house: wait on the HOST for the oldest copy
                self._buffers.remove(s)
                if s.event is not None:
                    s.event.synchronize()
            s = Staging(max(int(nbytes * 1.25), 1 << 20), torch.cuda.is_available())
            s.held = True
            self._buffers.append(s)
            return s

    def release(self, s):
        with self._lock:
            s.held = False

    def clear(self):
        with self._lock:
            self._buffers.clear()


# ---- encoders: batch geometry, plans, the fetch of the files ----
def batch_geometry(images, who):
    """(dtype code, N, H, W, element strides (n, c, y, x)) of an (N,H,W,3) uint8 or (N,3,H,W) float32 / bfloat16 batch."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"{who}: images must be a 4-d tensor, (N,H,W,3) uint8 or (N,3,H,W) float32 / bfloat16")
    if images.dtype == torch.uint8:
        if images.shape[3] != 3:
            raise ValueError(f"{who}: a uint8 batch is (N,H,W,3), got {tuple(images.shape)}")
        sn, sy, sx, sc = images.stride()
        return U8, images.shape[0], images.shape[1], images.shape[2], (sn, sc, sy, sx)
    if images.dtype in (torch.float32, torch.bfloat16):
        if images.shape[1] != 3:
            raise ValueError(f"{who}: a float batch is (N,3,H,W), got {tuple(images.shape)}")
        sn, sc, sy, sx = images.stride()
        return (_lib.F32 if images.dtype == torch.float32 else _lib.BF16), images.shape[0], images.shape[2], images.shape[3], (sn, sc, sy, sx)
    raise ValueError(f"{who}: dtype {images.dtype} is not uint8 / float32 / bfloat16")


def check_sizes(n, hmax, wmax, sizes, strides, who):
    """``sizes`` of a batch of that geometry as a list of int pairs (default: every image fills the batch); refuses an empty batch,
    sizes outside the batch and negative strides."""
    if n < 1 or hmax < 1 or wmax < 1:
        raise ValueError(f"{who}: empty batch")
    if sizes is None:
        sizes = [(hmax, wmax)] * n
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(sizes) != n or any(not (1 <= h <= hmax and 1 <= w <= wmax) for h, w in sizes):
        raise ValueError(f"{who}: sizes must be {n} pairs (h, w) inside the batch's {hmax} x {wmax}")
    if any(s < 0 for s in strides):
        raise ValueError(f"{who}: negative strides")
    return sizes


class PlanCache:
    """Per-geometry device state of the encoder ``who`` (``uploads``, sent once and reused -- also by a captured graph), oldest out."""
    def __init__(self, who, uploads, limit=64):
        self.who, self.uploads, self.limit = who, uploads, int(limit)
        self._plans = {}

    def __len__(self):
        return len(self._plans)

    def __contains__(self, key):
        return key in self._plans

    def get(self, key, build):
        """The plan of ``key``; ``build()`` makes a missing one, which uploads and is therefore refused inside a capture."""
        plan = self._plans.get(key)
        if plan is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self.who}.launch: this batch geometry has not been launched yet -- run launch once outside the "
                                   f"capture (it uploads {self.uploads}), then capture")
            plan = build()
            if len(self._plans) >= self.limit:                        # a stream of ever-changing geometries must not grow without bound
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = plan
        return plan


def fetch_packed(pool, out, stride, counts, indices=None):
    """list[bytes]: the first ``counts[i]`` bytes of slot i (at ``out[i * stride:]``) for i in ``indices`` (default: every slot).  One
    copy of exactly the used bytes into a staging buffer of ``pool`` on the current stream, waited for here."""
    indices = range(len(counts)) if indices is None else indices
    if not len(indices):
        return []
    used = sum(counts[i] for i in indices)
    st = pool.acquire(used)
    try:
        parts = [out[i * stride:i * stride + counts[i]] for i in indices]
        packed = parts[0] if len(parts) == 1 else torch.cat(parts)
        st.tensor[:used].copy_(packed, non_blocking=True)            # exactly the used bytes
        ev = torch.cuda.Event()
        ev.record()
        st.event = ev
        ev.synchronize()
        files, at = [], 0
        for i in indices:
            files.append(st.array[at:at + counts[i]].tobytes())
            at += counts[i]
    finally:
        pool.release(st)
    return files


class BatchFileEncoder:
    """The file writing of an encoder with ``launch(images, sizes)`` -> result with ``.out``, ``fetch(result)`` -> list[bytes] and
    ``encode_batch(images, sizes)``: a thread pool named ``prefix`` for the writes and, made on first use, one ``prefix``-io thread
    and one side stream for ``save_batch_async``.  ``who`` names the encoder in the error texts."""
    def _start_pool(self, threads, prefix, who):
        self.threads = worker_threads(threads)
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix=prefix)
        self._who, self._io_prefix = who, prefix + "-io"
        self._io = self._side = None          # background writer of save_batch_async: one thread, one side stream, made on first use
        self._io_lock = threading.Lock()

    def close(self):
        if self._io is not None:
            self._io.shutdown(wait=True)
        self._pool.shutdown(wait=True)

    def save_batch(self, images, paths, sizes=None):
        """Encode and write ``paths[i]``; returns the byte counts."""
        paths = self._check_paths(images, paths)
        files = self.encode_batch(images, sizes)
        list(self._pool.map(write, zip(paths, files)))
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
        with self._io_lock:
            if self._io is None:
                self._io = ThreadPoolExecutor(max_workers=1, thread_name_prefix=self._io_prefix)
                self._side = torch.cuda.Stream(device=res.out.device)
        return self._io.submit(self._finish_save, res, ev, paths)

    def _finish_save(self, res, ev, paths):
        with torch.cuda.device(res.out.device), torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            files = self.fetch(res)
        list(self._pool.map(write, zip(paths, files)))
        return [len(f) for f in files]

    def _check_paths(self, images, paths):
        paths = [os.fspath(p) for p in paths]
        if len(paths) != images.shape[0]:
            raise ValueError(f"{self._who}: {len(paths)} paths for {images.shape[0]} images")
        return paths


# ---- decoders: the batch on the host and its upload ----
class HostBatch:
    """A prepared batch in a staging buffer of ``pool``.  It owns the buffer until it is released (``release()`` or garbage
    collection), so it may be finished more than once."""
    def __init__(self, pool):
        self._pool = pool
        self.staging = None
        self.used = 0

    def release(self):
        if self.staging is not None:
            self._pool.release(self.staging)
            self.staging = None

    def __del__(self):
        try:
            self.release()
        except Exception:         # noqa: BLE001 -- interpreter shutdown
            pass


def upload(hb, device, who):
    """One non-blocking H2D copy of the used part of ``hb``'s staging buffer on ``device``'s current stream (the caller has made it
    the current device); the event guarding the buffer is recorded after it.  Returns the device buffer."""
    if hb.staging is None:
        raise RuntimeError(f"{who}: this HostBatch was released")
    buf = torch.empty(hb.used, dtype=torch.uint8, device=device)
    buf.copy_(hb.staging.tensor[:hb.used], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    hb.staging.event = ev
    return buf
