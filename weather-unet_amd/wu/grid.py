"""Image grids and tables on the GPU (csrc/grid.hip): ``torchvision.utils.make_grid(..., normalize=True, scale_each=True)`` of the pinned
torchvision (< 0.4) as the reference's drivers use it, in front of ``wu.jpeg_enc`` / ``wu.png_enc``.

* ``demo.py:74-82``: per angle, ``1 + num_classes`` one-column grids side by side, every cell normalised by its own min / max after
  ``(res + 1) * 127.5`` -- the frames of the GIF (``plan_demo_tables`` / ``demo_tables``);
* ``t_cls_train.py:361-378`` and ``t_est_train.py:342``: the evaluation summary, a blank and the reference images on top and one strip
  ``[image | its B transfers]`` per image, every strip normalised as a whole (``plan_summary`` / ``summary_image``);
* ``save_image`` called with a batch (``plan_grid`` / ``make_grid``).

A table is a list of CELLS: a (3, h, w) source image (fp32 or bf16, any strides), the frame it goes to and where, a normalisation
group, flags.  The planning functions are pure host code; ``GridComposer.compose`` binds a plan to its source tensors, uploads the
descriptors once per (plan, sources) and runs ``wu_grid_compose``: three launches whatever the number of cells and frames, no copy of
the sources, output either fp32 planar ``(F, 3, Hg, Wg)`` -- what ``make_grid`` returns -- or uint8 interleaved ``(F, Hg, Wg, 3)`` --
the batch the encoders take as it is.  The arithmetic is ``wu.infer_driver.normalize_minmax`` / ``to_uint8``'s, operation by operation
(include/wu_kernels.h), so the results equal the torch-op composition bit for bit.

    grid = make_grid(x, nrow=4, normalize=True, scale_each=True)      # (3, Hg, Wg) fp32
    frames = demo_tables(batch, axis_sweep(...))                      # (T, Hg, Wg, 3) uint8
"""
import ctypes
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from . import _lib
from .layout import stream_ptr

F_BF16, F_PRE, F_BLANK, F_NORMALIZE, F_FIXED_RANGE = 1, 2, 4, 8, 16          # WU_GRID_* flags
OUT_F32, OUT_U8 = 0, 1
_OUT = {"float": OUT_F32, "uint8": OUT_U8}

# One cell: ``source`` names an entry of the sources given to compose() (None: a blank cell), ``index`` the image inside it (a tuple over
# its leading dimensions); the cell covers rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of frame ``frame``; ``pre``: (x + 1) * 127.5
# first; ``normalize``: by the range of ``group``, or by ``value_range`` (lo, hi) when that is given.
Cell = namedtuple("Cell", "source index h w frame y0 x0 group pre normalize value_range")
# ``shape`` = (F, Hg, Wg); ``key`` identifies the geometry (the composer's cache)
Plan = namedtuple("Plan", "cells n_groups shape key")

CELL_DTYPE = np.dtype([("src", "<u8"), ("sc", "<i8"), ("sy", "<i8"), ("sx", "<i8"), ("h", "<i4"), ("w", "<i4"), ("frame", "<i4"),
                       ("y0", "<i4"), ("x0", "<i4"), ("group", "<i4"), ("flags", "<i4"), ("lo", "<f4"), ("hi", "<f4"), ("reserved", "<i4")])


def _range(value_range):
    if value_range is None:
        return None
    if not isinstance(value_range, tuple) or len(value_range) != 2:
        raise ValueError("value_range must be a tuple (min, max)")
    return (float(value_range[0]), float(value_range[1]))


def plan_grid(n, h, w, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False):
    """torchvision 0.3's ``make_grid`` loop for ``n`` images of h x w: ``xmaps = min(nrow, n)``, ``ymaps = ceil(n / xmaps)``, image k at
    ``(y (h + padding) + padding, x (w + padding) + padding)`` of a ``(h + padding) ymaps + padding`` by ``(w + padding) xmaps + padding``
    grid; the cells of a ragged last row stay at pad_value; ``n == 1`` is the image alone, no border.  ``scale_each``: one group per image,
    else one for the batch.  Source name: ``"x"``, index ``(k,)``."""
    n, h, w, nrow, padding = int(n), int(h), int(w), int(nrow), int(padding)
    if n < 1 or h < 1 or w < 1 or nrow < 1 or padding < 0:
        raise ValueError(f"plan_grid: bad geometry n={n} h={h} w={w} nrow={nrow} padding={padding}")
    vr = _range(value_range)                                          # checked here, in front of the cache: a list is a ValueError
    return _plan_grid(n, h, w, nrow, padding, bool(normalize), vr if normalize else None, bool(scale_each))


@lru_cache(maxsize=256)
def _plan_grid(n, h, w, nrow, padding, normalize, vr, scale_each):
    key = ("grid", n, h, w, nrow, padding, normalize, vr, scale_each)

    def cell(k, y0, x0):
        return Cell("x", (k,), h, w, 0, y0, x0, k if scale_each else 0, False, normalize, vr)
    if n == 1:
        return Plan((cell(0, 0, 0),), 1, (1, h, w), key)
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    height, width = h + padding, w + padding
    cells, k = [], 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            cells.append(cell(k, y * height + padding, x * width + padding))
            k += 1
    return Plan(tuple(cells), n if scale_each else 1, (1, height * ymaps + padding, width * xmaps + padding), key)


@lru_cache(maxsize=64)
def plan_demo_tables(T, nc, B, h, w):
    """demo.py:74-82 for T angles: per frame ``make_grid(batch, nrow=1, normalize=True, scale_each=True)`` and, per class axis a,
    ``make_grid((res + 1) * 127.5, nrow=1, normalize=True, scale_each=True)``, concatenated along the width -- ``1 + nc`` columns of B
    cells, every cell its own group, the pre-transform on for the result columns only.  Frame (3, B (h + 2) + 2, (1 + nc)(w + 4)); with
    B == 1 every grid is the image alone (make_grid's early return) and the frame is (3, h, (1 + nc) w).  Sources: ``"batch"`` (B, 3, h, w),
    index (b,); ``"results"`` (T, nc, B, 3, h, w) -- ``axis_sweep``'s output --, index (t, a, b)."""
    T, nc, B, h, w = int(T), int(nc), int(B), int(h), int(w)
    if min(T, nc, B, h, w) < 1:
        raise ValueError(f"plan_demo_tables: bad geometry T={T} nc={nc} B={B} h={h} w={w}")
    pad = 2 if B > 1 else 0
    hg, wcol = B * (h + pad) + pad, w + 2 * pad
    cells, g = [], 0
    for t in range(T):
        for col in range(1 + nc):
            for b in range(B):
                y0, x0 = b * (h + pad) + pad, col * wcol + pad
                if col == 0:
                    cells.append(Cell("batch", (b,), h, w, t, y0, x0, g, False, True, None))
                else:
                    cells.append(Cell("results", (t, col - 1, b), h, w, t, y0, x0, g, True, True, None))
                g += 1
    return Plan(tuple(cells), g, (T, hg, (1 + nc) * wcol), ("demo", T, nc, B, h, w))


@lru_cache(maxsize=64)
def plan_summary(B, h, w):
    """t_cls_train.py:361-378 (t_est_train.py:342): ``res_img`` is B + 1 strips of B + 1 images side by side without a gap -- strip 0 the
    blank (zeros_like(images[0])) and the B reference images, strip j + 1 ``images[j]`` and ``fakes[0][j] .. fakes[B - 1][j]`` -- and the
    picture ``make_grid(res_img, nrow=1, normalize=True, scale_each=True)``: the strips stacked with padding 2, each normalised as a whole
    (the blank's zeros count in strip 0's range).  Frame (3, (B + 1)(h + 2) + 2, (B + 1) w + 4).  Sources: ``"ref"`` (B, 3, h, w) index
    (i,), ``"images"`` (B, 3, h, w) index (j,), ``"fakes"`` (B, B, 3, h, w) -- what ``WeatherTransferStep.evaluation`` returns -- index (i, j)."""
    B, h, w = int(B), int(h), int(w)
    if min(B, h, w) < 1:
        raise ValueError(f"plan_summary: bad geometry B={B} h={h} w={w}")
    cells = []
    for s in range(B + 1):
        y0 = s * (h + 2) + 2
        for k in range(B + 1):
            x0 = 2 + k * w
            if s == 0:
                src, idx = (None, ()) if k == 0 else ("ref", (k - 1,))
            else:
                src, idx = ("images", (s - 1,)) if k == 0 else ("fakes", (k - 1, s - 1))
            cells.append(Cell(src, idx, h, w, 0, y0, x0, s, False, True, None))
    return Plan(tuple(cells), B + 1, (1, (B + 1) * (h + 2) + 2, (B + 1) * w + 4), ("summary", B, h, w))


def _require_cuda(t, what):
    if not t.is_cuda or not torch.cuda.is_available():
        raise RuntimeError(f"{what}: grids are composed by HIP kernels on an MI355X only -- got a {t.device} tensor. There is no CPU "
                           "fallback (wu.grid.plan_grid / plan_demo_tables / plan_summary are the host-only entry points)")


def _signature(sources):
    sig = []
    for name in sorted(sources):
        s = sources[name]
        for t in (s if isinstance(s, (list, tuple)) else (s,)):
            sig.append((name, t.data_ptr(), tuple(t.shape), t.stride(), t.dtype))
    return tuple(sig)


def _template(plan):
    """What a plan's descriptors hold whatever the sources are, and per source name the rows that take its pointers:
    (descriptors, {name: (rows, indices (n, k))})."""
    desc = np.zeros(len(plan.cells), dtype=CELL_DTYPE)
    by_source = {}
    for i, c in enumerate(plan.cells):
        flags = (F_NORMALIZE if c.normalize else 0) | (F_PRE if c.pre else 0)
        if c.source is None:
            flags |= F_BLANK
        else:
            rows, idx = by_source.setdefault(c.source, ([], []))
            if idx and len(idx[0]) != len(c.index):
                raise ValueError(f"grid: cell {i} indexes {c.source} with {len(c.index)} numbers, earlier cells with {len(idx[0])}")
            rows.append(i)
            idx.append(c.index)
        if c.normalize and c.value_range is not None:
            flags |= F_FIXED_RANGE
            desc[i]["lo"], desc[i]["hi"] = c.value_range
        desc[i]["flags"] = flags
    for f in ("h", "w", "frame", "y0", "x0", "group"):
        desc[f] = [getattr(c, f) for c in plan.cells]
    return desc, {name: (np.asarray(rows), np.asarray(idx, dtype=np.int64).reshape(len(rows), -1)) for name, (rows, idx) in by_source.items()}


class _Desc:
    """The uploaded descriptors of one (plan, sources): read-only on the device, so every stream and every captured graph may share
    them.  ``streams``: the streams they were used on besides the one that allocated them (``record_stream``: the allocator hands the
    memory out again only once their work is done); ``pinned``: a captured graph holds their address, they are never dropped."""
    def __init__(self, tensor, stream):
        self.tensor, self.streams, self.pinned = tensor, {stream}, False


class GridComposer:
    """Composes planned tables on the GPU.  ``compose`` runs on the CURRENT stream.  The descriptors of a (plan, sources) pair -- the
    pointers and strides of the source tensors are part of them -- are uploaded on the first call: that call holds the HOST until the
    copy of ``72 * n_cells`` bytes is done (it comes from pageable memory); every later call with the same tensors, overwritten in
    place or not, finds them cached and neither copies nor synchronises.  Tensors that are new on every call (``axis_sweep`` returns
    fresh ones) hit the cache only while the allocator hands the same addresses out again; otherwise each call pays the upload.

    Lifetimes.  The cache drops the descriptors used longest ago beyond ``MAX_CACHED`` pairs; memory used on a stream other than the
    one that allocated it is marked with ``record_stream``, so dropping it while kernels are in flight is safe.  The workspace (the
    range slots) belongs to a (size, stream) pair: composes on two streams never share one.  In a ``torch.cuda.graph`` capture --
    possible once the pair has been composed outside a capture, since the upload is a copy from pageable memory -- the descriptors
    used are PINNED: the graph holds their address, so they stay for the life of the composer, however many other pairs follow; the
    workspace and the output of a captured call come from the graph's own memory pool and live as long as the graph.  The sources of
    the last call are kept alive until the next one."""
    MAX_CACHED = 64

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._desc = {}                                                # (plan key, sources signature) -> _Desc, in order of last use
        self._ws = {}                                                  # (device index, bytes, stream) -> workspace
        self._templates = {}
        self._held = None
        self._lib = _lib.load()
        assert self._lib.wu_grid_cell_bytes() == CELL_DTYPE.itemsize

    def _describe(self, plan, sources):
        """The descriptors of ``plan`` over ``sources`` as a numpy record array: the plan's template (cached per geometry) with the
        pointers and strides of every cell's image worked out from its source tensor, no view per cell."""
        tpl = self._templates.get(plan.key)
        if tpl is None:
            if len(self._templates) >= self.MAX_CACHED:
                self._templates.pop(next(iter(self._templates)))
            tpl = self._templates[plan.key] = _template(plan)
        desc = tpl[0].copy()
        for name, (rows, idx) in tpl[1].items():
            if name not in sources:
                raise KeyError(f"grid: the plan reads from {name!r}, sources has {sorted(sources)}")
            s = sources[name]
            if isinstance(s, (list, tuple)):                           # a list of images: the index picks the tensor
                if idx.shape[1] != 1 or idx.min() < 0 or idx.max() >= len(s):
                    raise IndexError(f"grid: {name} is a list of {len(s)} images, the plan indexes it with {idx.shape[1]} numbers up to {idx.max()}")
                first = s[0]
                if any(t.dtype != first.dtype or t.shape != first.shape or t.device != first.device for t in s):
                    raise ValueError(f"grid: the images of {name} differ in type, size or device")
                lead = ()
                ptr = np.array([t.data_ptr() for t in s], dtype=np.uint64)[idx[:, 0]]
                strides = np.array([t.stride() for t in s], dtype=np.int64).reshape(len(s), -1)[idx[:, 0]]
            else:
                first, k = s, idx.shape[1]
                lead = tuple(s.shape[:max(s.dim() - 3, 0)])
                if len(lead) != k or (k and ((idx < 0).any() or (idx >= np.asarray(lead)).any())):
                    raise IndexError(f"grid: the plan indexes {name} with {k} numbers up to {idx.max(0).tolist() if k else []}, "
                                     f"its leading dimensions are {list(lead)}")
                off = idx @ np.asarray(s.stride()[:k], dtype=np.int64) if k else np.zeros(len(rows), dtype=np.int64)
                ptr = (np.int64(s.data_ptr()) + off * s.element_size()).astype(np.uint64)
                strides = np.broadcast_to(np.asarray(s.stride()[k:], dtype=np.int64), (len(rows), 3))
            if first.dim() != len(lead) + 3 or first.shape[-3] != 3 or (desc["h"][rows] != first.shape[-2]).any() or (desc["w"][rows] != first.shape[-1]).any():
                i = int(rows[0])
                raise ValueError(f"grid: cell {i} wants a (3, {desc['h'][i]}, {desc['w'][i]}) image from {name}, whose images are "
                                 f"{tuple(first.shape[len(lead):])}")
            if first.dtype == torch.bfloat16:
                desc["flags"][rows] |= F_BF16
            elif first.dtype != torch.float32:
                raise TypeError(f"grid: sources must be float32 or bfloat16, got {first.dtype}")
            if first.device != self.device and not (self.device.index is None and first.is_cuda):
                raise ValueError(f"grid: source on {first.device}, composer on {self.device}")
            desc["src"][rows] = ptr
            desc["sc"][rows], desc["sy"][rows], desc["sx"][rows] = strides[:, 0], strides[:, 1], strides[:, 2]
        return desc

    def _bind(self, plan, sources, device):
        """-> (descriptors, workspace, offset of the (lo, hi) pairs) for a compose on the current stream."""
        n, g = len(plan.cells), plan.n_groups
        ws_bytes = int(self._lib.wu_grid_workspace_bytes(n, g))
        if ws_bytes == 0:
            raise ValueError(f"grid: cannot compose {n} cells in {g} groups")
        off = (ctypes.c_longlong * 2)()
        _lib.call("wu_grid_workspace_layout", n, g, off)
        capturing = torch.cuda.is_current_stream_capturing()
        stream = torch.cuda.current_stream(device)
        key = (plan.key, _signature(sources))
        d = self._desc.pop(key, None)
        if d is None:
            if capturing:
                raise RuntimeError("GridComposer.compose: this plan has not been composed from these tensors yet -- run compose once "
                                   "outside the capture (it uploads the descriptors), then capture")
            d = _Desc(torch.from_numpy(self._describe(plan, sources).view(np.uint8).reshape(-1)).to(device), stream.cuda_stream)
        self._desc[key] = d                                            # last used, last dropped
        if capturing:
            d.pinned = True                                            # the graph replays from this address
        elif stream.cuda_stream not in d.streams:
            d.tensor.record_stream(stream)
            d.streams.add(stream.cuda_stream)
        if len(self._desc) > self.MAX_CACHED:                          # ever-changing sources must not grow the cache without bound
            for k, v in self._desc.items():
                if not v.pinned and v is not d:
                    del self._desc[k]
                    break
        if capturing:                                                  # from the graph's pool: owned by the graph, not by the cache
            return d.tensor, torch.empty(ws_bytes, dtype=torch.uint8, device=device), int(off[0])
        wkey = (device.index, ws_bytes, stream.cuda_stream)
        ws = self._ws.get(wkey)
        if ws is None:
            if len(self._ws) >= self.MAX_CACHED:                       # allocated and used on one stream only: freeing it is stream-ordered
                self._ws.pop(next(iter(self._ws)))
            ws = self._ws[wkey] = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        return d.tensor, ws, int(off[0])

    def compose(self, plan, sources, out="uint8", pad_value=0.0):
        """``sources``: {name: tensor or list of tensors} as the plan's cells name them (a bare tensor or list is ``{"x": ...}``).
        Returns (F, Hg, Wg, 3) uint8 or (F, 3, Hg, Wg) float32."""
        if out not in _OUT:
            raise ValueError(f"grid: out must be 'uint8' or 'float', got {out!r}")
        if not isinstance(sources, dict):
            sources = {"x": sources}
        tensors = [t for s in sources.values() for t in (s if isinstance(s, (list, tuple)) else (s,))]
        if not tensors:
            raise ValueError("grid: no sources")
        for t in tensors:
            _require_cuda(t, "GridComposer.compose")
        device = tensors[0].device
        f, hg, wg = plan.shape
        with torch.cuda.device(device):
            desc, ws, pairs_off = self._bind(plan, sources, device)
            if out == "uint8":
                res = torch.empty((f, hg, wg, 3), dtype=torch.uint8, device=device)
            else:
                res = torch.empty((f, 3, hg, wg), dtype=torch.float32, device=device)
            _lib.call("wu_grid_compose", desc.data_ptr(), len(plan.cells), plan.n_groups, ws.data_ptr(), ws.numel(), res.data_ptr(),
                      res.numel() * res.element_size(), _OUT[out], f, hg, wg, float(pad_value), stream_ptr())
        self._held = (sources, desc, ws, pairs_off, plan.n_groups)
        return res

    def ranges(self):
        """The (n_groups, 2) fp32 (lo, hi) pairs of the last compose, read through ``wu_grid_workspace_layout`` (tests, tools): a view
        of its workspace, valid until the next compose on the same stream.  Groups that no normalising cell uses hold zeros."""
        _, _, ws, pairs_off, n_groups = self._held
        return ws[pairs_off:pairs_off + 8 * n_groups].view(torch.float32).view(-1, 2)


_composers = {}


def composer(device):
    """One shared GridComposer per device, created on first use."""
    device = torch.device(device)
    c = _composers.get(device)
    if c is None:
        c = _composers[device] = GridComposer(device)
    return c


def _images(tensor):
    """make_grid's input forms -> (source, n, h, w); grey input is out of scope."""
    if isinstance(tensor, (list, tuple)):
        if not tensor or not all(torch.is_tensor(t) for t in tensor):
            raise TypeError("make_grid: a tensor or a list of tensors")
        if any(t.dim() != 3 or t.shape != tensor[0].shape for t in tensor):
            raise ValueError("make_grid: a list holds (3, H, W) images of one size")
        src, n, shape = list(tensor), len(tensor), tensor[0].shape
    elif torch.is_tensor(tensor):
        if tensor.dim() == 3:
            tensor = tensor.unsqueeze(0)
        if tensor.dim() != 4:
            raise ValueError(f"make_grid: (B, 3, H, W), (3, H, W) or a list of (3, H, W), got {tuple(tensor.shape)}")
        src, n, shape = tensor, tensor.shape[0], tensor.shape[1:]
    else:
        raise TypeError(f"make_grid: tensor or list of tensors expected, got {type(tensor)}")
    if shape[0] != 3:
        raise ValueError(f"make_grid: three-channel images only (grey input is not supported), got {shape[0]} channels")
    return src, n, int(shape[1]), int(shape[2])


def _first(src):
    return src[0] if isinstance(src, list) else src


@torch.no_grad()
def compose_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0, out="float", **kw):
    """``make_grid`` with the output kind open: ``out="uint8"`` gives the (Hg, Wg, 3) bytes ``save_image`` writes."""
    if "range" in kw:                                                  # torchvision < 0.4's name of the argument
        value_range = kw.pop("range")
    if kw:
        raise TypeError(f"make_grid: unexpected arguments {sorted(kw)}")
    src, n, h, w = _images(tensor)
    _require_cuda(_first(src), "make_grid")
    plan = plan_grid(n, h, w, nrow, padding, normalize, value_range, scale_each)
    return composer(_first(src).device).compose(plan, {"x": src}, out, pad_value)[0]


def make_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0, **kw):
    """``torchvision.utils.make_grid`` (< 0.4; ``range=`` is accepted for ``value_range=``) on the GPU: (B, 3, H, W), (3, H, W) or a list
    of (3, H, W) images, fp32 or bf16, any strides, not copied.  Returns fp32 (3, Hg, Wg)."""
    return compose_grid(tensor, nrow, padding, normalize, value_range, scale_each, pad_value, "float", **kw)


@torch.no_grad()
def demo_tables(batch, results, out="uint8"):
    """The frames of demo.py:67-92: ``batch`` (B, 3, H, W), ``results`` (T, nc, B, 3, H, W) -- ``wu.infer_driver.axis_sweep``'s raw
    output, not copied.  Returns (T, Hg, Wg, 3) uint8, or (T, 3, Hg, Wg) fp32 with ``out="float"``.  One call, three launches."""
    _require_cuda(results, "demo_tables")
    if results.dim() != 6 or batch.dim() != 4 or results.shape[3] != 3 or tuple(results.shape[2:]) != tuple(batch.shape):
        raise ValueError(f"demo_tables: batch (B,3,H,W) and results (T,nc,B,3,H,W), got {tuple(batch.shape)} and {tuple(results.shape)}")
    T, nc, B, _, h, w = results.shape
    return composer(results.device).compose(plan_demo_tables(T, nc, B, h, w), {"batch": batch, "results": results}, out)


@torch.no_grad()
def summary_image(images, ref_images, fakes, out="float"):
    """The ``images/test`` picture of t_cls_train.py:361-378: ``images`` and ``ref_images`` (B, 3, H, W), ``fakes`` (B, B, 3, H, W) as
    ``WeatherTransferStep.evaluation`` returns them.  Returns fp32 (3, Hg, Wg), or (Hg, Wg, 3) uint8 with ``out="uint8"``."""
    _require_cuda(fakes, "summary_image")
    B = images.shape[0]
    if images.dim() != 4 or images.shape[1] != 3 or ref_images.shape != images.shape or tuple(fakes.shape) != (B, B) + tuple(images.shape[1:]):
        raise ValueError(f"summary_image: images / ref_images (B,3,H,W) and fakes (B,B,3,H,W), got {tuple(images.shape)}, "
                         f"{tuple(ref_images.shape)}, {tuple(fakes.shape)}")
    plan = plan_summary(B, images.shape[2], images.shape[3])
    return composer(fakes.device).compose(plan, {"images": images, "ref": ref_images, "fakes": fakes}, out)[0]
