"""Colour-transfer baselines: what a method that can ONLY move colours reaches on the project's evaluation.  Per-channel histogram matching
and its N-dimensional form, the iterative distribution transfer of Pitie, Kokaram and Dahyot (2005 / 2007), i.e. sliced optimal transport
(Rabin et al. 2011; Bonneel et al. 2015), take every photograph to the colour distribution of real photographs of a target class.

    pal = ClassPalettes.from_dirs({"snowy": "data/snowy", "rainy": "data/rainy"}, P=65536, size=224)
    y = transfer(x, pal, targets=[0, 1])                # (B, 3, H, W) -> (R, B, 3, H, W), like Conditional_UNet.sweep
    ClassTransferEval(ColourBaseline(pal), classifier, nc, content=..., swd=..., lpips=...)
    y = transfer(x, pal, targets=[0, 1], method="mkl", regrain=True)     # the linear Monge-Kantorovich map, then regraining
    z = regrain(x, y)                                   # the regraining pass on its own: y's colours, x's gradients
    python -m wu.colour SRC_DIR OUT_DIR (--palettes P.npz | --class NAME=DIR ...) [--iters K] [--size S] [--points P] [--seed N]
                        [--save-palettes P.npz] [--ext .png|.jpg] [--method idt|meanstd|mkl] [--regrain] [--regrain-smoothness S]

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

K = 1 is exact per-channel histogram matching, the classic baseline; K = 20 (the default) is the N-dimensional transfer.

Linear maps (``method="meanstd"`` / ``"mkl"``, beside the default ``"idt"``; ``iters``, ``seed`` and ``step`` are ignored by them).  With
(mu_s, Sigma_s) the mean and population covariance of the image's n states and (mu_t, Sigma_t) those of the palette -- two passes, every sum
in an order fixed by the number of addends alone (include/wu_kernels.h) -- ``s <- mu_t + A (s - mu_s)``, evaluated as
``((A_c0 d_0 + A_c1 d_1) + A_c2 d_2) + mu_t_c``.  ``meanstd`` (Reinhard et al. 2001, in the input's RGB):
``A = diag(sqrt(Sigma_t_cc / max(Sigma_s_cc, EPS_VAR)))``.  ``mkl`` (the linear Monge-Kantorovich map, Pitie & Kokaram 2007):
``A = Sigma_s^(-1/2) (Sigma_s^(1/2) Sigma_t Sigma_s^(1/2))^(1/2) Sigma_s^(-1/2)``, the eigenvalues of Sigma_s floored at EPS_VAR = 1e-10
([0, 1]^2 units: the variance of 8-bit quantisation is 1.3e-6, so only flat images meet the floor), those under the inner root at 0.  Matrix
functions come from a cyclic Jacobi of exactly 8 sweeps with no trigonometry, on the device: nothing is read back.

Regraining (``regrain=True`` or a ``Regrain(iters, smoothness, min_side)``; Pitie, Kokaram and Dahyot 2007, section 5).  The iterated
transfer stretches the colour map locally, so sensor noise or JPEG blocks of a flat sky come out as grain and banding.  The pass keeps the
transferred colours IT and gives the result the gradient field of the original I0: a multigrid Jacobi solve between the last iteration
(or the linear map) and the store, on the unclipped state.  include/wu_kernels.h states the rule (levels, down, up, weights, iteration);
tests/_regrain_ref.py restates it.  One deliberate departure from the published code: the coarse solution CORRECTS the finer iterate,
``IR = IR + up(c1 - down(IR))``, where that code replaces it by ``up(c1)`` -- with IT = I0 the correction form returns I0 to 1.6e-15 where the
replacement form leaves 1.5e-2 at edges.  ``regrain(original, transferred)`` is the same pass for anything that
should keep a photograph's grain, the generator's own sweep included.

OUT OF SCOPE: edge-aware post-filters other than this regraining, any colour space other than the input's RGB, signal-conditioned (estimator)
baselines, and images beyond 2^21 pixels -- run at the network's S x S and, if wanted, pass the result through ``wu.guided`` as the
drivers do for the generator.

Kernels (csrc/colour_ot.hip): the state stays on the GPU as (images, 3, n) float64; every iteration projects it, sorts the 3 columns of
every image with the segmented sort of ``wu.swd``, and one fused kernel recomputes each pixel's keys, finds lo / hi by bisection in the
sorted column (the first steps in an LDS sample of it), looks up the palette quantile and writes the new state.  Palette keys are sorted
once per iteration, not per image.  No atomics: two runs give the same bits, and ``max_images`` changes memory only.  CUDA tensors only:
there is no CPU fallback.  csrc/colour_regrain.hip holds the moments, the linear map and the regraining kernels: the solve keeps a tile of all
three channels in LDS and runs up to 8 iterations per launch on a halo of as many cells, or all iterations of a level of at most 4096 pixels."""
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
METHODS = {"idt": None, "meanstd": 0, "mkl": 1}      # the `mode` of wu_colour_linear_apply
EPS_VAR = 1e-10                          # the floor of the source variances of the linear maps, in [0, 1]^2 units
MAX_SETS = 65535                         # point sets of one wu_colour_moments / wu_colour_linear_apply call
REGRAIN_ITERS = (4, 16, 32, 64, 64, 64)


class Regrain:
    """The parameters of the regraining pass: ``iters`` a tuple of 1 to 6 positive iteration counts, finest level first; ``smoothness`` > 0
    (larger keeps more of the original's gradients where they are strong); a coarser level exists while both halved sides exceed
    ``min_side`` >= 0."""

    def __init__(self, iters=REGRAIN_ITERS, smoothness=1.0, min_side=20):
        try:
            it = tuple(iters)
        except TypeError:
            raise ValueError(f"Regrain: iters must be a tuple of 1 to 6 positive ints, got {iters!r}") from None
        if not 1 <= len(it) <= 6 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 or int(v) > 1 << 20 for v in it):
            raise ValueError(f"Regrain: iters must be a tuple of 1 to 6 positive ints (at most 2^20 each), got {iters!r}")
        smoothness = float(smoothness)
        if not 0.0 < smoothness < float("inf"):
            raise ValueError(f"Regrain: smoothness {smoothness} must be positive and finite")
        if isinstance(min_side, bool) or int(min_side) != min_side or int(min_side) < 0:
            raise ValueError(f"Regrain: min_side {min_side!r} must be an int >= 0")
        self.iters, self.smoothness, self.min_side = tuple(int(v) for v in it), smoothness, int(min_side)

    def __repr__(self):
        return f"Regrain(iters={self.iters}, smoothness={self.smoothness}, min_side={self.min_side})"


def _regrain_arg(regrain):
    if regrain is None or regrain is False:
        return None
    if regrain is True:
        return Regrain()
    if isinstance(regrain, Regrain):
        return regrain
    raise ValueError(f"regrain must be None, True or a Regrain(...), got {regrain!r}")


class _RegrainPlan:
    """The level count, host iteration array and device workspace of a regraining pass over chunks of at most ``chunk`` images of h x w."""

    def __init__(self, rg, chunk, h, w, dev, what):
        lib = _lib.load()
        self.levels = lib.wu_colour_regrain_levels(h, w, len(rg.iters), rg.min_side)
        nbytes = lib.wu_colour_regrain_workspace_bytes(chunk, h, w, self.levels)
        if self.levels < 1 or nbytes == 0:
            raise ValueError(f"{what}: {chunk} images of {h} x {w}: out of the regraining kernels' range")
        self.iters = (ctypes.c_int * self.levels)(*rg.iters[:self.levels])
        self.smoothness, self.h, self.w = rg.smoothness, h, w
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.original = torch.empty((chunk, 3, h * w), dtype=torch.float64, device=dev)

    def run(self, state, cnt, sp):
        _lib.call("wu_colour_regrain", state.data_ptr(), self.original.data_ptr(), cnt, self.h, self.w, self.levels, self.iters,
                  self.smoothness, self.ws.data_ptr(), sp)


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

    def moments(self, device):
        """(C, 12) float64 on ``device``: mean and covariance of every palette (wu_colour_moments), made once per device and kept."""
        cache = self.__dict__.setdefault("_moments", {})
        key = str(device)
        if key not in cache:
            C, P = self.num_classes, self.P
            lib = _lib.load()
            nbytes = lib.wu_colour_moments_workspace_bytes(C, P)
            if nbytes == 0:
                raise ValueError(f"ClassPalettes: {C} palettes of {P} points: out of the moment kernels' range")
            pal = self.palettes.to(device)
            out = torch.empty((C, 12), dtype=torch.float64, device=device)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                _lib.call("wu_colour_moments", pal.data_ptr(), 3, 1, C, P, out.data_ptr(), ws.data_ptr(), stream_ptr())
            cache[key] = out
        return cache[key]

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


def transfer(x, palettes, targets, iters=20, seed=0, step=1.0, value_range=(-1, 1), max_images=None, method="idt", regrain=None):
    """x (B, 3, H, W) -> (R, B, 3, H, W) of x's dtype: every image taken to the palette of every class index in ``targets`` (R,).
    ``method="idt"`` (the default): ``iters`` iterations of the module docstring's rule; ``iters=1`` is per-channel histogram matching.
    ``method="meanstd"`` / ``"mkl"``: the closed-form linear maps; ``iters``, ``seed`` and ``step`` are ignored by them.  ``regrain``: None
    (the default), True (the defaults) or a ``Regrain(...)``: the original state of every chunk is loaded a second time and the regraining
    pass runs between the last iteration (or the linear map) and the store.  ``palettes``: a ``ClassPalettes`` (or a (C, P, 3) tensor, which
    is then checked on every call).  ``max_images`` bounds how many of the R B images are in flight and changes memory only.  Bad values
    raise before any launch; once the arguments are checked (a ``targets`` tensor on the device is read back for that) nothing synchronises
    with the host: every launch goes on the current stream."""
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
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"transfer: method {method!r} must be one of {sorted(METHODS)}")
    rg = _regrain_arg(regrain)
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
    idt = method == "idt"
    if idt:
        nbytes = lib.wu_colour_ot_workspace_bytes(chunk, n, C, P)
    else:
        chunk = min(chunk, MAX_SETS)
        nbytes = lib.wu_colour_moments_workspace_bytes(chunk, n) if lib.wu_colour_moments_workspace_bytes(C, P) else 0
    if nbytes == 0:
        raise ValueError(f"transfer: {chunk} images of {n} pixels, {C} palettes of {P} points: out of the kernels' range")
    plan = _RegrainPlan(rg, chunk, h, w, dev, "transfer") if rg is not None else None
    cls = _class_index(str(dev), tuple(tg), b)
    out = torch.empty((r, b, 3, h, w), dtype=x.dtype, device=dev)
    state = torch.empty((chunk, 3, n), dtype=torch.float64, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dt = _DTYPES[x.dtype]
    if idt:
        rots = draw_rotations(seed, iters)
        rot_c = [(ctypes.c_double * 9)(*rots[k].reshape(-1).tolist()) for k in range(iters)]
        # palette keys depend on (class, k) alone: with one chunk of images they are made as the iterations go, with several they are kept
        keep = chunk < total and iters * C * 3 * P * 8 <= KEY_BYTES
        keys = torch.empty((iters if keep else 1, C * 3, P), dtype=torch.float64, device=dev)
    else:
        pal_mom = pal.moments(dev)
        mom = torch.empty((chunk, 12), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        sp = stream_ptr()

        def palette_keys(k, slot):
            _lib.call("wu_colour_ot_palette_keys", pal_d.data_ptr(), C, P, rot_c[k], keys[slot].data_ptr(), ws.data_ptr(), sp)

        if idt and keep:
            for k in range(iters):
                palette_keys(k, k)
        for first in range(0, total, chunk):
            cnt = min(chunk, total - first)
            _lib.call("wu_colour_ot_load", x.data_ptr(), *x.stride(), dt, b, h, w, scale, shift, L, first, cnt, state.data_ptr(), sp)
            if plan is not None:
                _lib.call("wu_colour_ot_load", x.data_ptr(), *x.stride(), dt, b, h, w, scale, shift, L, first, cnt, plan.original.data_ptr(),
                          sp)
            if idt:
                for k in range(iters):
                    if not keep:
                        palette_keys(k, 0)
                    _lib.call("wu_colour_ot_step", state.data_ptr(), cnt, n, keys[k if keep else 0].data_ptr(), C, P, cls[first:].data_ptr(),
                              rot_c[k], float(step), ws.data_ptr(), sp)
            else:
                _lib.call("wu_colour_moments", state.data_ptr(), 1, n, cnt, n, mom.data_ptr(), ws.data_ptr(), sp)
                _lib.call("wu_colour_linear_apply", state.data_ptr(), cnt, n, mom.data_ptr(), pal_mom.data_ptr(), C, cls[first:].data_ptr(),
                          METHODS[method], EPS_VAR, sp)
            if plan is not None:
                plan.run(state, cnt, sp)
            _lib.call("wu_colour_ot_store", state.data_ptr(), first, cnt, out.data_ptr(), *out.stride(), dt, b, h, w, lo, span, round_int, sp)
    return out


def regrain(original, transferred, value_range=(-1, 1), iters=REGRAIN_ITERS, smoothness=1.0, min_side=20, max_images=None):
    """The regraining pass on its own: the colours of ``transferred`` with the gradient field of ``original``.  ``original`` (B, 3, H, W)
    against ``transferred`` (B, 3, H, W) or (R, B, 3, H, W) -- a sweep of the generator or of ``transfer`` -- each float32, bfloat16 or
    uint8 of any strides, both in ``value_range``.  Returns the dtype and shape of ``transferred``, clipped to the range as ``transfer``
    clips.  ``max_images`` bounds the images in flight and changes memory only."""
    rg = Regrain(iters, smoothness, min_side)
    if not torch.is_tensor(original) or original.dim() != 4 or original.shape[1] != 3 or original.shape[0] < 1:
        raise ValueError(f"regrain: original must be (B, 3, H, W), got {tuple(getattr(original, 'shape', ()))}")
    if not torch.is_tensor(transferred) or transferred.dim() not in (4, 5) or tuple(transferred.shape[-4:]) != tuple(original.shape) \
            or transferred.shape[0] < 1:
        raise ValueError(f"regrain: transferred must be {tuple(original.shape)} or (R,) + that, got {tuple(getattr(transferred, 'shape', ()))}")
    if original.dtype not in _DTYPES or transferred.dtype not in _DTYPES:
        raise ValueError(f"regrain: float32, bfloat16 or uint8, got {original.dtype} and {transferred.dtype}")
    b, _, h, w = original.shape
    n = h * w
    if not 1 <= n <= MAX_N:
        raise ValueError(f"regrain: H W = {n} out of 1..{MAX_N}; run at the network's size")
    if max_images is not None and int(max_images) < 1:
        raise ValueError(f"regrain: max_images {max_images} must be at least 1")
    scale, shift, L = range_mapping(value_range)
    if not original.is_cuda or transferred.device != original.device:
        raise RuntimeError("wu.colour: CUDA tensors on one device only -- no CPU fallback")
    if isinstance(value_range, str):
        lo, span, round_int = 0.0, 255.0, 1
    else:
        lo, span, round_int = float(value_range[0]), float(value_range[1]) - float(value_range[0]), 0
    x, y = original.detach(), transferred.detach()
    y5 = y if y.dim() == 5 else y.unsqueeze(0)
    dev = x.device
    chunk = b if max_images is None else min(b, int(max_images))
    plan = _RegrainPlan(rg, chunk, h, w, dev, "regrain")
    out = torch.empty(y5.shape, dtype=y.dtype, device=dev)
    state = torch.empty((chunk, 3, n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        sp = stream_ptr()
        for r in range(y5.shape[0]):
            yr = y5[r]
            for first in range(0, b, chunk):
                cnt = min(chunk, b - first)
                _lib.call("wu_colour_ot_load", x.data_ptr(), *x.stride(), _DTYPES[x.dtype], b, h, w, scale, shift, L, first, cnt,
                          plan.original.data_ptr(), sp)
                _lib.call("wu_colour_ot_load", yr.data_ptr(), *yr.stride(), _DTYPES[y.dtype], b, h, w, scale, shift, L, first, cnt,
                          state.data_ptr(), sp)
                plan.run(state, cnt, sp)
                _lib.call("wu_colour_ot_store", state.data_ptr(), r * b + first, cnt, out.data_ptr(), *out.stride(), _DTYPES[y.dtype], b, h,
                          w, lo, span, round_int, sp)
    return out if y.dim() == 5 else out[0]


class ColourBaseline:
    """The colour-transfer baseline behind the interface the evaluators are written against: ``sweep(batch, rows, max_images)`` with
    one-hot ``rows`` (R, C), as ``ClassTransferEval`` passes them, returns (R, B, 3, H, W); row r goes to the palette of its arg-max.  A row
    that is not one-hot raises: signal rows have no palette."""

    def __init__(self, palettes, iters=20, seed=0, value_range=(-1, 1), method="idt", regrain=None):
        self.palettes = palettes if isinstance(palettes, ClassPalettes) else ClassPalettes(palettes)
        self.iters, self.seed, self.value_range = int(iters), seed, value_range
        if not isinstance(method, str) or method not in METHODS:
            raise ValueError(f"ColourBaseline: method {method!r} must be one of {sorted(METHODS)}")
        self.method, self.regrain = method, _regrain_arg(regrain)

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
        return transfer(batch, self.palettes, rows.argmax(1).tolist(), self.iters, self.seed, 1.0, self.value_range, max_images, self.method,
                        self.regrain)


# ----------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------
def transfer_dir(src_dir, out_dir, palettes, iters=20, size=None, seed=0, ext=".png", batch_size=16, device="cuda:0", method="idt",
                 regrain=None):
    """Every .jpg / .png file of ``src_dir`` to every class: ``out_dir/NAME/<stem><ext>`` through ``wu.infer_driver.save_images``.
    ``method`` and ``regrain`` as in ``transfer``.  Returns the number of images read."""
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
        out = transfer(x, palettes, list(range(palettes.num_classes)), iters, seed, 1.0, rng, None, method, regrain)
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
    ap.add_argument("--method", default="idt", choices=sorted(METHODS), help="idt: the iterated transfer; meanstd / mkl: the closed-form "
                    "linear maps, which ignore --iters and --seed's rotations")
    ap.add_argument("--regrain", action="store_true", help="finish with the regraining pass (the original's gradients under the new colours)")
    ap.add_argument("--regrain-smoothness", type=float, default=None, metavar="S", help="smoothness of the regraining pass (implies --regrain)")
    args = ap.parse_args(argv)
    rg = None
    if args.regrain or args.regrain_smoothness is not None:
        try:
            rg = Regrain(smoothness=1.0 if args.regrain_smoothness is None else args.regrain_smoothness)
        except ValueError as e:
            ap.error(str(e))
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
    n = transfer_dir(args.src_dir, args.out_dir, pal, args.iters, args.size, args.seed, args.ext, method=args.method, regrain=rg)
    torch.cuda.synchronize()
    how = f"method idt, K {args.iters}" if args.method == "idt" else f"method {args.method}"
    grain = "regrain off" if rg is None else f"regrain on (smoothness {rg.smoothness:g})"
    print(f"Colour: {n} images, {pal.num_classes} classes, {how}, P {pal.P}, {grain}, {time.perf_counter() - t0:.2f} s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
