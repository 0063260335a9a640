"""Colour-transfer baselines: what a method that can ONLY move colours reaches on the project's evaluation.  Per-channel histogram matching
and its N-dimensional form, the iterative distribution transfer of Pitie, Kokaram and Dahyot (2005 / 2007), i.e. sliced optimal transport
(Rabin et al. 2011; Bonneel et al. 2015), take every photograph to the colour distribution of real photographs of a target class.

    pal = ClassPalettes.from_dirs({"snowy": "data/snowy", "rainy": "data/rainy"}, P=65536, size=224)
    y = transfer(x, pal, targets=[0, 1])                # (B, 3, H, W) -> (R, B, 3, H, W), like Conditional_UNet.sweep
    ClassTransferEval(ColourBaseline(pal), classifier, nc, content=..., swd=..., lpips=...)
    python -m wu.colour SRC_DIR OUT_DIR (--palettes P.npz | --class NAME=DIR ...) [--iters K] [--size S] [--points P] [--seed N]
                        [--save-palettes P.npz] [--ext .png|.jpg]

Semantics, in full (tests/_colour_ref.py restates them in numpy).  All arithmetic in float64, every operation rounded on its own, no FMA.

Input.  ``x`` (B, 3, H, W), float32, bfloat16 or uint8, any strides; ``n = H W`` with 1 <= n <= 2^21.  With
``(scale, shift, L) = wu.paired.range_mapping(value_range)`` a value v becomes the state ``s = (double(v) scale + shift) / L``: [0, 1]
units for every dtype.

Palette.  ``palette`` (C, P, 3) float64 in the same units, 1 <= P <= 2^21: P real pixels per class.  Duplicates are allowed, values must
be finite.

Rotations (``draw_rotations(seed, K)`` -> float64 (K, 3, 3), on the host).  ``R_0 = I``; for k >= 1, with one
``rng = np.random.RandomState(seed)`` for the whole sequence, ``A = rng.randn(3, 3)``, ``Q, T = np.linalg.qr(A)``,
``Q = Q * np.sign(np.diag(T))``, ``R_k = Q.T``.  Row a of R_k is axis a; R_k does not depend on K.  The kernels take the matrices as
input.

One iteration k, for one image and the palette of its target class, R = R_k.  Every pixel and every palette point is projected onto each
axis a: ``key_a = (R[a][0] s_0 + R[a][1] s_1) + R[a][2] s_2``; ``q_a`` is the ascending sort of the P palette keys of axis a.  For each
pixel, among the n keys of axis a of ITS image: ``lo = #{key' < key}``, ``hi = #{key' <= key}``, ``t = ((lo + hi) P) // (2 n)`` in int64
(always in [0, P - 1], since 1 <= lo + hi <= 2 n - 1), ``delta_a = q_a[t] - key_a``.  Then per channel c:
``d_c = (delta_0 R[0][c] + delta_1 R[1][c]) + delta_2 R[2][c]`` and ``s_c = s_c + step d_c``.  The state is not clipped between
iterations.  This is a mid-rank rule: equal colours stay equal (a flat sky stays flat), and no tie-break or stability of the sort can show.

Output.  After K iterations ``u = min(max(s, 0), 1)``.  A float range (lo, hi): ``v = lo + u (hi - lo)``, rounded float64 -> float32 and
float32 -> bfloat16 for bf16 outputs, both to nearest-even.  ``"uint8"``: ``rint(u 255)``, half to even (a uint8 tensor under a float range
is rounded the same way).  The output dtype is the input's.

K = 1 is exact per-channel histogram matching, the classic baseline; K = 20 (the default) is the N-dimensional transfer.  OUT OF SCOPE:
regraining and any edge-aware post-filter, the linear Monge-Kantorovich map, mean / sigma (Reinhard) transfer, any colour space other than
the input's RGB, signal-conditioned (estimator) baselines, and images beyond 2^21 pixels -- run at the network's S x S and, if wanted,
pass the result through ``wu.guided`` as the drivers do for the generator.

Kernels (csrc/colour_ot.hip): the state stays on the GPU as (images, 3, n) float64; every iteration projects it, sorts the 3 columns of
every image with the segmented sort of ``wu.swd``, and one fused kernel recomputes each pixel's keys, finds lo / hi by bisection in the
sorted column (the first steps in an LDS sample of it), looks up the palette quantile and writes the new state.  Palette keys are sorted
once per iteration, not per image.  No atomics: two runs give the same bits, and ``max_images`` changes memory only.  CUDA tensors only:
there is no CPU fallback."""
import ctypes
import functools
import os
import time

import numpy as np
import torch

from . import _lib
from .layout import stream_ptr
from .paired import U8, range_mapping

MAX_N = 1 << 21                         # pixels of an image, points of a palette
KEY_BYTES = 1 << 30                     # with several chunks of images in a call, the sorted palette keys of all iterations are kept if they fit
_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: U8}


def draw_rotations(seed, K):
    """float64 (K, 3, 3): R_0 = I, then Haar-distributed rotations from one RandomState(seed); the first K of any longer draw."""
    K = int(K)
    if K < 1:
        raise ValueError(f"draw_rotations: K {K} must be at least 1")
    rng = np.random.RandomState(seed)
    out = np.empty((K, 3, 3), dtype=np.float64)
    out[0] = np.eye(3)
    for k in range(1, K):
        A = rng.randn(3, 3)
        Q, T = np.linalg.qr(A)
        Q = Q * np.sign(np.diag(T))
        out[k] = Q.T
    return out


def draw_points(seed, N, H, W, P):
    """The P pixels a palette takes from N images of H x W: (i, y, x) int64 arrays, drawn in that order from RandomState(seed)."""
    if min(int(N), int(H), int(W), int(P)) < 1:
        raise ValueError(f"draw_points: N {N}, H {H}, W {W}, P {P} must all be at least 1")
    rng = np.random.RandomState(seed)
    i = rng.randint(0, N, P)
    y = rng.randint(0, H, P)
    x = rng.randint(0, W, P)
    return i.astype(np.int64), y.astype(np.int64), x.astype(np.int64)


def _gather(images, i, y, x, value_range):
    scale, shift, L = range_mapping(value_range)
    dev = images.device
    v = images[torch.from_numpy(i).to(dev), :, torch.from_numpy(y).to(dev), torch.from_numpy(x).to(dev)].to(torch.float64)
    # a DEVICE tensor as divisor: by a Python number torch multiplies with the reciprocal on the GPU, which is not the quotient's rounding
    return (v * scale + shift) / torch.full((1,), L, dtype=torch.float64, device=dev)


def palette_from_images(images, P, seed=0, value_range=(-1, 1)):
    """(P, 3) float64 in [0, 1] units, on the images' device: pixel (i, y, x) of ``draw_points(seed, N, H, W, P)`` of an (N, 3, H, W) batch
    (float32, bfloat16 or uint8).  A torch gather: this is not the hot path."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError(f"palette_from_images: an (N, 3, H, W) batch, got {tuple(getattr(images, 'shape', ()))}")
    if not 1 <= int(P) <= MAX_N:
        raise ValueError(f"palette_from_images: P {P} out of 1..{MAX_N}")
    n, _, h, w = images.shape
    return _gather(images.detach(), *draw_points(seed, n, h, w, int(P)), value_range)


class ClassPalettes:
    """(C, P, 3) float64 palettes in [0, 1] units, one per class, with the classes' names and how they were drawn.  The values are checked
    here, once (finite; a device tensor is read back for that), so that ``transfer`` does not have to."""

    def __init__(self, palettes, names=None, seed=None, sources=None):
        p = palettes if torch.is_tensor(palettes) else torch.from_numpy(np.ascontiguousarray(palettes, dtype=np.float64))
        if p.dim() != 3 or p.shape[2] != 3 or p.shape[0] < 1:
            raise ValueError(f"ClassPalettes: (C, P, 3) palettes, got {tuple(p.shape)}")
        if not 1 <= p.shape[1] <= MAX_N:
            raise ValueError(f"ClassPalettes: P {p.shape[1]} out of 1..{MAX_N}")
        p = p.detach().to(torch.float64).contiguous()
        if not bool(torch.isfinite(p).all()):
            raise ValueError("ClassPalettes: palette values must be finite")
        self.palettes = p
        self.names = [str(v) for v in names] if names is not None else [str(c) for c in range(p.shape[0])]
        if len(self.names) != p.shape[0]:
            raise ValueError(f"ClassPalettes: {len(self.names)} names for {p.shape[0]} classes")
        self.seed, self.sources = seed, list(sources) if sources is not None else None

    num_classes = property(lambda self: self.palettes.shape[0])
    P = property(lambda self: self.palettes.shape[1])

    def to(self, device):
        if self.palettes.device != torch.device(device):
            self.palettes = self.palettes.to(device)
        return self

    def save_npz(self, path):
        np.savez(path, palettes=self.palettes.cpu().numpy(), names=np.array(self.names), P=self.P,
                 seed=-1 if self.seed is None else int(self.seed), sources=np.array([str(s) for s in self.sources or []]))

    @classmethod
    def load_npz(cls, path, device=None):
        with np.load(path) as f:
            seed = int(f["seed"])
            out = cls(f["palettes"], f["names"].tolist(), None if seed < 0 else seed, f["sources"].tolist())
        return out.to(device) if device is not None else out

    @classmethod
    def from_dirs(cls, dirs, P=65536, size=None, seed=0, batch_size=64, gpu_decode=False, device="cuda:0"):
        """One palette per entry of ``{name: directory}``: P pixels of the directory's .jpg / .png files, read as wu.swd / wu.fid read
        them and resized to size x size by the loader's rule (without ``size`` all files of a class must have one size).  The files go
        through in sorted order and the pixels are ``draw_points(seed, N, H, W, P)`` of the whole class, so the palette does not depend on
        ``batch_size``."""
        from .files import image_files, read_images
        pals = []
        for name, d in dirs.items():
            files = image_files(d)
            if not files:
                raise RuntimeError(f"no .jpg / .png images in {d}")
            pal, pts, at = None, None, 0
            for x, rng in read_images(files, size, gpu_decode, device, batch_size):
                if pts is None:
                    i, y, xx = draw_points(seed, len(files), x.shape[2], x.shape[3], int(P))
                    pts, hw = (i, y, xx), tuple(x.shape[2:])
                    pal = torch.empty(int(P), 3, dtype=torch.float64, device=x.device)
                elif tuple(x.shape[2:]) != hw:
                    raise ValueError(f"images of different sizes in {d} ({hw} and {tuple(x.shape[2:])}): give size")
                take = np.nonzero((pts[0] >= at) & (pts[0] < at + x.shape[0]))[0]
                if take.size:
                    pal[torch.from_numpy(take).to(x.device)] = _gather(x, pts[0][take] - at, pts[1][take], pts[2][take], rng)
                at += x.shape[0]
            pals.append(pal)
        return cls(torch.stack(pals), list(dirs), seed, [os.fspath(d) for d in dirs.values()])


def _target_list(targets, C):
    t = targets.detach().cpu().tolist() if torch.is_tensor(targets) else list(targets)
    if not t or any(isinstance(v, (list, tuple)) for v in t):
        raise ValueError("transfer: targets must be a non-empty (R,) list or tensor of class indices")
    if any(int(v) != v for v in t):
        raise ValueError(f"transfer: targets must be integers, got {t}")
    t = [int(v) for v in t]
    if min(t) < 0 or max(t) >= C:
        raise ValueError(f"transfer: targets {t} must be in 0..{C - 1}; nothing is clamped")
    return t


@functools.lru_cache(maxsize=64)
def _class_index(device, targets, B):
    """int32 (R B): the class of virtual image r B + b, on the device.  Cached: a repeated call uploads nothing."""
    return torch.tensor([t for t in targets for _ in range(B)], dtype=torch.int32).to(device)


def transfer(x, palettes, targets, iters=20, seed=0, step=1.0, value_range=(-1, 1), max_images=None):
    """x (B, 3, H, W) -> (R, B, 3, H, W) of x's dtype: every image taken to the palette of every class index in ``targets`` (R,) by ``iters``
    iterations of the module docstring's rule; ``iters=1`` is per-channel histogram matching.  ``palettes``: a ``ClassPalettes`` (or a
    (C, P, 3) tensor, which is then checked on every call).  ``max_images`` bounds how many of the R B images are in flight and changes
    memory only.  Once the arguments are checked (a ``targets`` tensor on the device is read back for that) nothing synchronises with the
    host: every launch goes on the current stream."""
    pal = palettes if isinstance(palettes, ClassPalettes) else ClassPalettes(palettes)
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError(f"transfer: x must be (B, 3, H, W), got {tuple(getattr(x, 'shape', ()))}")
    if x.dtype not in _DTYPES:
        raise ValueError(f"transfer: float32, bfloat16 or uint8, got {x.dtype}")
    b, _, h, w = x.shape
    n, C, P = h * w, pal.num_classes, pal.P
    if not 1 <= n <= MAX_N:
        raise ValueError(f"transfer: H W = {n} out of 1..{MAX_N}; run at the network's size")
    iters = int(iters)
    if iters < 1:
        raise ValueError(f"transfer: iters {iters} must be at least 1")
    if max_images is not None and int(max_images) < 1:
        raise ValueError(f"transfer: max_images {max_images} must be at least 1")
    tg = _target_list(targets, C)
    scale, shift, L = range_mapping(value_range)
    if not x.is_cuda:
        raise RuntimeError("wu.colour: CUDA tensors only -- no CPU fallback")
    if isinstance(value_range, str):
        lo, span, round_int = 0.0, 255.0, 1
    else:
        lo, span, round_int = float(value_range[0]), float(value_range[1]) - float(value_range[0]), 0
    x = x.detach()
    dev = x.device
    pal_d = pal.palettes.to(dev)
    r, total = len(tg), len(tg) * b
    chunk = total if max_images is None else min(total, int(max_images))
    lib = _lib.load()
    nbytes = lib.wu_colour_ot_workspace_bytes(chunk, n, C, P)
    if nbytes == 0:
        raise ValueError(f"transfer: {chunk} images of {n} pixels, {C} palettes of {P} points: out of the kernels' range")
    rots = draw_rotations(seed, iters)
    rot_c = [(ctypes.c_double * 9)(*rots[k].reshape(-1).tolist()) for k in range(iters)]
    cls = _class_index(str(dev), tuple(tg), b)
    out = torch.empty((r, b, 3, h, w), dtype=x.dtype, device=dev)
    state = torch.empty((chunk, 3, n), dtype=torch.float64, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # palette keys depend on (class, k) alone: with one chunk of images they are made as the iterations go, with several they are kept
    keep = chunk < total and iters * C * 3 * P * 8 <= KEY_BYTES
    keys = torch.empty((iters if keep else 1, C * 3, P), dtype=torch.float64, device=dev)
    dt = _DTYPES[x.dtype]
    with torch.cuda.device(dev):
        sp = stream_ptr()

        def palette_keys(k, slot):
            _lib.call("wu_colour_ot_palette_keys", pal_d.data_ptr(), C, P, rot_c[k], keys[slot].data_ptr(), ws.data_ptr(), sp)

        if keep:
            for k in range(iters):
                palette_keys(k, k)
        for first in range(0, total, chunk):
            cnt = min(chunk, total - first)
            _lib.call("wu_colour_ot_load", x.data_ptr(), *x.stride(), dt, b, h, w, scale, shift, L, first, cnt, state.data_ptr(), sp)
            for k in range(iters):
                if not keep:
                    palette_keys(k, 0)
                _lib.call("wu_colour_ot_step", state.data_ptr(), cnt, n, keys[k if keep else 0].data_ptr(), C, P, cls[first:].data_ptr(),
                          rot_c[k], float(step), ws.data_ptr(), sp)
            _lib.call("wu_colour_ot_store", state.data_ptr(), first, cnt, out.data_ptr(), *out.stride(), dt, b, h, w, lo, span, round_int, sp)
    return out


class ColourBaseline:
    """The colour-transfer baseline behind the interface the evaluators are written against: ``sweep(batch, rows, max_images)`` with
    one-hot ``rows`` (R, C), as ``ClassTransferEval`` passes them, returns (R, B, 3, H, W); row r goes to the palette of its arg-max.  A row
    that is not one-hot raises: signal rows have no palette."""

    def __init__(self, palettes, iters=20, seed=0, value_range=(-1, 1)):
        self.palettes = palettes if isinstance(palettes, ClassPalettes) else ClassPalettes(palettes)
        self.iters, self.seed, self.value_range = int(iters), seed, value_range

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def sweep(self, batch, rows, max_images=None):
        rows = rows.detach().cpu() if torch.is_tensor(rows) else torch.as_tensor(np.asarray(rows))
        C = self.palettes.num_classes
        if rows.dim() != 2 or rows.shape[0] < 1 or rows.shape[1] != C:
            raise ValueError(f"ColourBaseline.sweep: rows must be (R, {C}) one-hot, got {tuple(rows.shape)}")
        rows = rows.to(torch.float64)
        if not bool((((rows == 1).sum(1) == 1) & ((rows == 0).sum(1) == C - 1)).all()):
            raise ValueError("ColourBaseline.sweep: every row must be one-hot (signal rows have no palette)")
        return transfer(batch, self.palettes, rows.argmax(1).tolist(), self.iters, self.seed, 1.0, self.value_range, max_images)


# ----------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------
def transfer_dir(src_dir, out_dir, palettes, iters=20, size=None, seed=0, ext=".png", batch_size=16, device="cuda:0"):
    """Every .jpg / .png file of ``src_dir`` to every class: ``out_dir/NAME/<stem><ext>`` through ``wu.infer_driver.save_images``.
    Returns the number of images read."""
    from .files import image_files, read_images
    from .infer_driver import save_images
    files = image_files(src_dir)
    if not files:
        raise RuntimeError(f"no .jpg / .png images in {src_dir}")
    for name in palettes.names:
        os.makedirs(os.path.join(out_dir, name), exist_ok=True)
    palettes.to(device)
    at = 0
    for x, rng in read_images(files, size, False, device, batch_size):
        out = transfer(x, palettes, list(range(palettes.num_classes)), iters, seed, 1.0, rng)
        # the writers take [0, 1] floats and truncate v * 255: a byte b goes in as (b + 0.5) / 255, the middle of its bucket
        out01 = (out.float() + 0.5) / 255 if isinstance(rng, str) else (out.float() - rng[0]) / (rng[1] - rng[0])
        part = files[at:at + x.shape[0]]
        for c, name in enumerate(palettes.names):
            save_images(out01[c], [os.path.join(out_dir, name, f.stem + ext) for f in part], normalize=False)
        at += x.shape[0]
    return at


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wu.colour", description="colour-transfer baseline: every image of SRC_DIR taken to the "
                                 "colour distribution of every class, OUT_DIR/NAME/<file>")
    ap.add_argument("src_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--palettes", default=None, help="a .npz written by --save-palettes")
    ap.add_argument("--class", dest="classes", action="append", default=[], metavar="NAME=DIR", help="a class and its directory of real images")
    ap.add_argument("--iters", type=int, default=20, help="iterations; 1 is per-channel histogram matching")
    ap.add_argument("--size", type=int, default=None, help="resize every image to SIZE x SIZE first (the loader's rule)")
    ap.add_argument("--points", type=int, default=65536, help="pixels per class palette")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save-palettes", default=None)
    ap.add_argument("--ext", default=".png", choices=[".png", ".jpg"])
    args = ap.parse_args(argv)
    if bool(args.palettes) == bool(args.classes):
        ap.error("give either --palettes P.npz or one --class NAME=DIR per class")
    if args.palettes:
        pal = ClassPalettes.load_npz(args.palettes)
    else:
        dirs = {}
        for kv in args.classes:
            name, sep, d = kv.partition("=")
            if not sep or not name or not d:
                ap.error(f"--class {kv!r}: NAME=DIR")
            dirs[name] = d
        pal = ClassPalettes.from_dirs(dirs, args.points, args.size, args.seed)
    if args.save_palettes:
        pal.save_npz(args.save_palettes)
    t0 = time.perf_counter()
    n = transfer_dir(args.src_dir, args.out_dir, pal, args.iters, args.size, args.seed, args.ext)
    torch.cuda.synchronize()
    print(f"Colour: {n} images, {pal.num_classes} classes, K {args.iters}, P {pal.P}, {time.perf_counter() - t0:.2f} s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
