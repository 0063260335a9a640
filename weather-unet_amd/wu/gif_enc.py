"""GIF encoding of the demo animation (csrc/gif_enc.hip): the palette and the LZW of ``wu.infer_driver.save_demo(frames, "x.gif")`` on
the GPU, so that what crosses to the host is the finished image blocks instead of every frame as raw RGB.

Per frame, independently: a 32768-bin histogram over the top 5 bits of each channel, median cut over the occupied bins down to at most 256
boxes, palette entry = rounded mean of its box, index = the box of the pixel's bin (no dithering, no nearest-colour search); then GIF LZW
over segments of 8192 indices that each start from the fresh dictionary, their bit strings joined bit by bit.  Every distinct frame is
quantised and coded ONCE; the host puts ``GIF89a``, the logical screen descriptor, the loop extension and the trailer around the blocks
and repeats a block wherever ``order`` names its frame again (the ping-pong of demo.py names all but two frames twice).

The files are NOT the bytes Pillow writes (another palette order, one unsegmented LZW): Pillow decodes them to ``palette[index]``, and they
equal ``tests/_gif_enc_ref.encode`` byte for byte.  The output buffer is sized by the exact worst case (every pixel a 12-bit code), so there
is no overflow and no Pillow fallback.

Limitation of the defaults: colours are told apart by their histogram bin, so an image with several distinct colours in one 5-bit bin is
not reproduced exactly even if it has 256 colours or fewer (a 256-level grey ramp comes out at about 41 dB, where Pillow is exact), a smooth
ramp comes out in bands, and every frame has a palette of its own.  The options lift each of these (all integer rules, restated in
``tests/_gif_quality_ref.py``; they change the file, so they are opt-in):

    mapping="nearest"   index = the nearest palette entry in use (squared distance in 8-bit RGB, lowest index among equals), not the bin's box
    dither="ordered"    an 8 x 8 ordered dither in front of that search, from the pixel's position only (so it does not flicker between
                        frames), at most one step of the local palette and at most 16 levels; needs mapping="nearest"
    exact=True          a frame (or, under a global palette, an animation) of at most 256 colours keeps exactly those colours
    palette="global"    one palette for all frames in a global colour table: a cell that does not change keeps its colours
    GPUGifEncoder.best(...)  all four

    enc = GPUGifEncoder()
    data = enc.encode(frames, duration_ms=125, loop=0, order=ping_pong(T))      # frames (T, H, W, 3) uint8 on the GPU; bytes
    enc.save(frames, "demo.gif", duration_ms=125, order=ping_pong(T))
"""
import os
import struct
import threading

import torch

from . import _codec, _lib
from .layout import stream_ptr


def ping_pong(t):
    """[0 .. t-1, t-2 .. 1]: the frame order of demo.py's animation."""
    t = int(t)
    return list(range(t)) + list(range(t - 2, 0, -1))


def segment_pixels():
    """Indices per LZW segment.  Host only."""
    return int(_lib.load().wu_gif_enc_segment_pixels())


def block_stride(h, w):
    """The exact worst case of an h x w image block: the distance between two frames' blocks in the output buffer.  Host only."""
    n = int(_lib.load().wu_gif_enc_block_stride(int(h), int(w)))
    if n == 0:
        raise ValueError(f"gif_enc: cannot encode {h} x {w} (at most 65535 on a side and 2^26 pixels)")
    return n


NEAREST, ORDERED, EXACT, GLOBAL = 1, 2, 4, 8     # the flags of wu_gif_enc_encode_ex


def option_flags(mapping="box", dither=None, exact=False, palette="local"):
    """The flags of a set of options; ValueError for anything else.  Host only."""
    if mapping not in ("box", "nearest"):
        raise ValueError(f"GPUGifEncoder: mapping must be 'box' or 'nearest', got {mapping!r}")
    if dither not in (None, "ordered"):
        raise ValueError(f"GPUGifEncoder: dither must be None or 'ordered', got {dither!r}")
    if exact is not True and exact is not False:
        raise ValueError(f"GPUGifEncoder: exact must be True or False, got {exact!r}")
    if palette not in ("local", "global"):
        raise ValueError(f"GPUGifEncoder: palette must be 'local' or 'global', got {palette!r}")
    if dither == "ordered" and mapping != "nearest":
        raise ValueError("GPUGifEncoder: dither='ordered' requires mapping='nearest'")
    return (NEAREST if mapping == "nearest" else 0) | (ORDERED if dither else 0) | (EXACT if exact else 0) | (GLOBAL if palette == "global" else 0)


class DeviceResult:
    """Result of GPUGifEncoder.launch: the image blocks on the device (frame t at ``out[t * block_stride:]``) and their byte counts in
    ``result``.  With options also ``info`` (T, 2) int32 -- palette entries in use and whether the frame took the exact path -- and, under
    a global palette, ``palette``: its 768 bytes."""
    def __init__(self, out, result, workspace, frames, t, h, w, stride, flags=0, palette=None, info=None):
        self.out, self.result, self.workspace, self.frames = out, result, workspace, frames
        self.t, self.h, self.w, self.block_stride = t, h, w, stride
        self.flags, self.palette, self.info = flags, palette, info


class GPUGifEncoder:
    """Animated-GIF encoder on the GPU.

    ``encode(frames, duration_ms, loop, order)`` = ``fetch(launch(frames), duration_ms, loop, order)``.  ``launch`` queues one memset and
    five kernels on the CURRENT stream and never synchronises; it holds no per-geometry device state, so it can be captured in a
    ``torch.cuda.graph`` as it is.  ``fetch`` does one small device-to-host copy of the T byte counts, then one copy of exactly the used
    bytes into a pinned staging buffer, and assembles the file: header, the blocks in ``order`` with the frame delay written into each,
    trailer.

    Staging buffers: ``wu._codec.StagingPool``.

    ``frames``: (T, H, W, 3) uint8 on the GPU, any non-negative strides (what ``wu.grid.demo_tables(..., out="uint8")`` returns).

    ``mapping``, ``dither``, ``exact``, ``palette``: the quality options of the module docstring (``wu_gif_enc_encode_ex``); the defaults
    write the bytes of ``tests/_gif_enc_ref.encode``, any option those of ``tests/_gif_quality_ref.encode``.  Under ``palette="global"``
    ``fetch`` also copies the 768 bytes of the palette for the header.  ``best()`` turns all four on.
    """
    def __init__(self, device="cuda", max_staging=4, mapping="box", dither=None, exact=False, palette="local"):
        self.flags = option_flags(mapping, dither, exact, palette)
        self.mapping, self.dither, self.exact, self.palette = mapping, dither, exact, palette
        self.device = torch.device(device)
        self.max_staging = int(max_staging)
        self._lock = threading.Lock()
        self._staging = _codec.StagingPool(self.max_staging)
        self.stats = {"frames": 0, "bytes": 0}
        self._lib = _lib.load()
        self.segment_pixels = int(self._lib.wu_gif_enc_segment_pixels())

    @classmethod
    def best(cls, device="cuda", max_staging=4):
        """Every quality option on: nearest-colour mapping, ordered dither, exact small palettes, one global palette."""
        return cls(device, max_staging, mapping="nearest", dither="ordered", exact=True, palette="global")

    def close(self):
        self._staging.clear()

    # ---- device stage ----
    def launch(self, frames):
        """The kernels on the current stream; returns a DeviceResult."""
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
            what = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, torch.Tensor) else type(frames).__name__
            raise ValueError(f"GPUGifEncoder: frames must be a (T, H, W, 3) uint8 tensor, got {what}")
        if not frames.is_cuda or not torch.cuda.is_available() or self.device.type != "cuda":
            raise RuntimeError("GPUGifEncoder: the encoder runs HIP kernels on an MI355X only -- there is no CPU fallback "
                               "(wu.gif_enc.block_stride / segment_pixels / ping_pong are the host-only entry points)")
        t, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if t < 1 or h < 1 or w < 1:
            raise ValueError("GPUGifEncoder: no frames")
        st, sy, sx, sc = frames.stride()
        if min(st, sy, sx, sc) < 0:
            raise ValueError("GPUGifEncoder: negative strides")
        flags = self.flags
        if flags == 0:                                                     # the defaults stay on the first entry points throughout
            stride, ws_bytes = int(self._lib.wu_gif_enc_block_stride(h, w)), int(self._lib.wu_gif_enc_workspace_bytes(t, h, w))
        else:
            stride = int(self._lib.wu_gif_enc_block_stride_ex(h, w, flags))
            ws_bytes = int(self._lib.wu_gif_enc_workspace_bytes_ex(t, h, w, flags))
        if stride == 0 or ws_bytes == 0:
            raise ValueError(f"GPUGifEncoder: cannot encode {t} frames of {h} x {w} (at most 65535 on a side and 2^26 pixels; under a "
                             "global palette fewer than 2^32 pixels in all)")
        palette = info = None
        with torch.cuda.device(frames.device):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=frames.device)
            out = torch.empty(t * stride, dtype=torch.uint8, device=frames.device)
            result = torch.empty(t, dtype=torch.int32, device=frames.device)
            if flags == 0:
                _lib.call("wu_gif_enc_encode", frames.data_ptr(), st, sy, sx, sc, ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                          result.data_ptr(), t, h, w, 0, stream_ptr())
            else:
                info = torch.empty((t, 2), dtype=torch.int32, device=frames.device)
                palette = torch.empty(768, dtype=torch.uint8, device=frames.device) if flags & GLOBAL else None
                _lib.call("wu_gif_enc_encode_ex", frames.data_ptr(), st, sy, sx, sc, ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                          result.data_ptr(), t, h, w, 0, flags, palette.data_ptr() if palette is not None else None, info.data_ptr(),
                          stream_ptr())
        return DeviceResult(out, result, ws, frames, t, h, w, stride, flags, palette, info)

    # ---- host stage ----
    def fetch(self, res, duration_ms, loop=0, order=None):
        """bytes: the GIF file of a launched batch of frames, shown in ``order`` (default 0 .. T-1) for ``duration_ms`` each (GIF counts
        1/100 s: ``duration_ms // 10``), repeated ``loop`` times (0: for ever; None: no loop extension, shown once)."""
        delay = int(duration_ms) // 10
        if not 0 <= delay <= 65535:
            raise ValueError(f"GPUGifEncoder: duration {duration_ms} ms outside 0 .. 655350")
        if loop is not None and not 0 <= int(loop) <= 65535:
            raise ValueError(f"GPUGifEncoder: loop count {loop} outside 0 .. 65535")
        order = list(range(res.t)) if order is None else [int(i) for i in order]
        if not order or any(not 0 <= i < res.t for i in order):
            raise ValueError(f"GPUGifEncoder: order must name frames 0 .. {res.t - 1}")
        with torch.cuda.device(res.out.device):
            counts = [int(c) for c in res.result.cpu().numpy()]          # the small copy: T byte counts
            if any(not 0 < c <= res.block_stride for c in counts):
                raise RuntimeError(f"GPUGifEncoder: byte counts {counts} outside (0, {res.block_stride}]")
            blocks = _codec.fetch_packed(self._staging, res.out, res.block_stride, counts)
        for i, b in enumerate(blocks):
            blocks[i] = b[:4] + struct.pack("<H", delay) + b[6:]         # the graphic control extension's delay
        if res.flags & GLOBAL:                                             # a 256-entry global colour table; the blocks carry none
            head = b"GIF89a" + struct.pack("<HH", res.w, res.h) + b"\xF7\x00\x00" + res.palette.cpu().numpy().tobytes()
        else:
            head = b"GIF89a" + struct.pack("<HH", res.w, res.h) + b"\x70\x00\x00"
        if loop is not None:
            head += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", int(loop)) + b"\x00"
        with self._lock:
            self.stats["frames"] += res.t
            self.stats["bytes"] += sum(counts)
        return head + b"".join(blocks[i] for i in order) + b"\x3B"

    def encode(self, frames, duration_ms, loop=0, order=None):
        return self.fetch(self.launch(frames), duration_ms, loop, order)

    def save(self, frames, path, duration_ms, loop=0, order=None):
        """Encode and write ``path``; returns the byte count."""
        data = self.encode(frames, duration_ms, loop, order)
        with open(os.fspath(path), "wb") as fh:
            fh.write(data)
        return len(data)
