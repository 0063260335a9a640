"""PNG encoding behind the inference and evaluation drivers (csrc/png_enc.hip): the lossless counterpart of ``wu.jpeg_enc``, for the
``.png`` variants of the reference's writers and for outputs that feed ``python -m wu.fid``, where JPEG artefacts bias the statistic.

Row filters (the minimum-sum-of-absolute-differences heuristic over the five PNG filters) and a literal-only dynamic-Huffman deflate
per 32 KiB segment of the filtered stream -- a stored block where that is not larger -- are parallel from end to end, so everything
runs on the GPU, checksums and framing included: three kernel launches per batch, and what crosses to the host is the finished files.
The files are 8-bit RGB, colour type 2, no interlace, no ancillary chunks.  They are NOT the bytes Pillow writes (Pillow runs zlib's
LZ77 matcher; these files are larger): they decode to the same pixels, and they equal ``tests/_png_enc_ref.encode`` byte for byte.
The output buffer is sized by the exact worst case (every segment stored), so there is no overflow and no Pillow fallback.

``GPUPngEncoder(matching="lz77")`` adds LZ77 matching for what a photograph does not have -- repeated cells, padding, flat or
clipped regions, smooth ramps (grids, demo tables, summary images): two more launches, per segment a block of literals and matches
that replaces the stored / literal-only one only where it is strictly smaller, so no file grows.  Those files equal
``tests/_png_lz_ref.encode``, where the matching rule is written down.  The default, ``matching="none"``, is the encoder as it was.

    enc = GPUPngEncoder()
    files = enc.encode_batch(images)                  # list[bytes]; images (N,H,W,3) uint8 or (N,3,H,W) fp32 / bf16 in [0, 1]
    enc.save_batch(images, paths)                     # the same bytes, written on the thread pool
    done = enc.save_batch_async(images, paths)        # ... without waiting: a Future; the next forward can be queued at once
"""
import threading

import numpy as np
import torch

from . import _codec, _lib
from ._codec import MAX_THREADS, U8  # noqa: F401 -- public names of this module; U8 is WU_PNG_ENC_U8
from .layout import stream_ptr


LZ77 = 1                                     # WU_PNG_ENC_LZ77: the flag of wu_png_enc_encode_ex


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
    def __init__(self, desc, ws_bytes, out_stride, n, hmax, wmax, info_offset=0, nseg_max=0, nseg=()):
        self.desc, self.ws_bytes, self.out_stride = desc, ws_bytes, out_stride
        self.n, self.hmax, self.wmax = n, hmax, wmax
        self.info_offset, self.nseg_max, self.nseg = info_offset, nseg_max, nseg       # where the segment info lies; segments per image


class DeviceResult:
    """Result of GPUPngEncoder.launch: the files on the device (image i at ``out[i * out_stride:]``) and their byte counts in
    ``result``."""
    def __init__(self, out, result, workspace, plan, images, sizes):
        self.out, self.result, self.workspace, self.plan = out, result, workspace, plan
        self.images, self.sizes = images, sizes
        self.n, self.out_stride = plan.n, plan.out_stride


class GPUPngEncoder(_codec.BatchFileEncoder):
    """Batch PNG encoder on the GPU.

    ``encode_batch(images, sizes)`` = ``fetch(launch(images, sizes))``.  ``launch`` runs the three kernels on the CURRENT stream and
    never synchronises; for a fixed batch geometry it can be captured in a ``torch.cuda.graph`` once one launch of that geometry has
    run outside the capture (that first launch uploads the descriptors).  ``fetch`` does one small device-to-host copy of the N byte
    counts, then one copy of exactly the used bytes into a pinned staging buffer.

    ``save_batch`` / ``save_batch_async`` / ``close``: ``wu._codec.BatchFileEncoder``.  Staging buffers: ``wu._codec.StagingPool``.

    ``images``: (N, H, W, 3) uint8, or (N, 3, H, W) float32 / bfloat16 with samples in [0, 1] (any strides: contiguous, channels-last,
    a slice ...), converted as ``wu.infer_driver.to_uint8`` does.  ``sizes``: [(h, w)] per image for a padded batch (what
    ``GPUJpegDecoder`` emits); the padding is never read.

    ``matching``: "none" (literal-only blocks, three launches) or "lz77" (five launches; see the module text).  ``stats`` counts the
    segments by the block they got -- "stored", "literal", "lz77", keys that appear with the first fetched batch -- from the segment
    info ``fetch`` copies with the byte counts.
    """
    MATCHING = {"none": 0, "lz77": LZ77}

    def __init__(self, device="cuda", threads=None, max_staging=8, matching="none"):
        if matching not in self.MATCHING:
            raise ValueError(f"GPUPngEncoder: matching={matching!r} is not one of {sorted(self.MATCHING)}")
        self.matching, self._flags = matching, self.MATCHING[matching]
        self.device = torch.device(device)
        self.max_staging = int(max_staging)
        self._start_pool(threads, "wu-png-enc", "GPUPngEncoder")
        self._lock = threading.Lock()         # guards stats
        self._staging = _codec.StagingPool(self.max_staging)
        self._plans = _codec.PlanCache("GPUPngEncoder", "the descriptors")
        self.stats = {"native": 0, "bytes": 0}        # and "stored" / "literal" / "lz77" from the first fetched batch on
        self._lib = _lib.load()
        assert self._lib.wu_png_enc_desc_bytes() == 16
        self.segment_bytes = int(self._lib.wu_png_enc_segment_bytes())

    # ---- device stage ----
    def _plan(self, n, hmax, wmax, sizes):
        return self._plans.get((n, hmax, wmax, tuple(sizes)), lambda: self._make_plan(n, hmax, wmax, sizes))

    def _make_plan(self, n, hmax, wmax, sizes):
        ws_bytes = int(self._lib.wu_png_enc_workspace_bytes_ex(n, hmax, wmax, self._flags))
        stride = int(self._lib.wu_png_enc_out_stride(hmax, wmax))
        if ws_bytes == 0 or stride == 0:
            raise ValueError(f"GPUPngEncoder: cannot encode a batch of {n} images of up to {hmax} x {wmax}")
        desc = np.zeros((n, 4), dtype=np.int32)
        desc[:, :2] = sizes
        seg = self.segment_bytes
        nseg = tuple(-(-h * (1 + 3 * w) // seg) for h, w in sizes)
        return _Plan(torch.from_numpy(desc).to(self.device), ws_bytes, stride, n, hmax, wmax,
                     int(self._lib.wu_png_enc_seginfo_offset(n, hmax, wmax)), -(-hmax * (1 + 3 * wmax) // seg), nseg)

    def launch(self, images, sizes=None):
        """The kernels on the current stream; returns a DeviceResult."""
        dt, n, hmax, wmax, strides = _codec.batch_geometry(images, "GPUPngEncoder")
        if not images.is_cuda or not torch.cuda.is_available() or self.device.type != "cuda":
            raise RuntimeError("GPUPngEncoder: the encoder runs HIP kernels on an MI355X only -- there is no CPU fallback "
                               "(wu.png_enc.out_stride / segment_bytes are the host-only entry points)")
        sizes = _codec.check_sizes(n, hmax, wmax, sizes, strides, "GPUPngEncoder")
        with torch.cuda.device(images.device):
            plan = self._plan(n, hmax, wmax, sizes)
            ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=images.device)
            out = torch.empty(n * plan.out_stride, dtype=torch.uint8, device=images.device)
            result = torch.empty(n, dtype=torch.int32, device=images.device)
            _lib.call("wu_png_enc_encode_ex", images.data_ptr(), dt, strides[0], strides[1], strides[2], strides[3], plan.desc.data_ptr(),
                      ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), result.data_ptr(), n, hmax, wmax, self._flags, stream_ptr())
        return DeviceResult(out, result, ws, plan, images, sizes)

    # ---- host stage ----
    def fetch(self, res):
        """list[bytes]: one complete PNG file per image of a launched batch."""
        with torch.cuda.device(res.out.device):
            counts = [int(c) for c in res.result.cpu().numpy()]          # the small copy: N byte counts
            plan = res.plan
            info = res.workspace[plan.info_offset:plan.info_offset + plan.n * plan.nseg_max * 16].view(torch.int32)
            modes = info.view(plan.n, plan.nseg_max, 4)[:, :, 3].cpu().numpy()       # ... and one word per segment: the block it got
            if any(not 0 < c <= res.out_stride for c in counts):
                raise RuntimeError(f"GPUPngEncoder: byte counts {counts} outside (0, {res.out_stride}]")
            files = _codec.fetch_packed(self._staging, res.out, res.out_stride, counts)
        with self._lock:
            self.stats["native"] += res.n
            self.stats["bytes"] += sum(counts)
            for i, k in enumerate(plan.nseg):
                for name, code in (("literal", 0), ("stored", 1), ("lz77", 2)):
                    self.stats[name] = self.stats.get(name, 0) + int((modes[i, :k] == code).sum())
        return files

    def encode_batch(self, images, sizes=None):
        return self.fetch(self.launch(images, sizes))
