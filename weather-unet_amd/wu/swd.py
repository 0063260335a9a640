"""Sliced Wasserstein distance (SWD) on Laplacian-pyramid patches (Karras et al. 2018, "Progressive growing of GANs", section 5 and its
``metrics/sliced_wasserstein.py``): one number per spatial scale that says how far the local texture statistics of two image sets are apart.
Pixels only: no pretrained network, no feature extractor.

    r = swd(images_a, images_b)                         # (N, 3, H, W) each -> SWDResult(levels=(.., .., ..) x 1e3, mean)
    d = descriptors(images, positions)                  # per level, (N * P, 147) float32 CUDA
    dn, mu, sigma = normalize(d[0])
    w = sliced_wasserstein(dn_a, dn_b, dirs)            # (ndirs,) float64 CUDA
    r = swd(images_a, images_b, unequal="exact")        # (Na, 3, H, W) against (Nb, 3, H, W): the exact W1 per direction, nothing dropped
    r = compare(DescriptorBank.from_dir(DIR_A), DescriptorBank.from_dir(DIR_B))
    python -m wu.swd DIR_A DIR_B [--size S [--filter bicubic]] [--patches 128] [--repeats 4] [--dirs 128] [--seed 0] [--gpu-decode]
                                 [--unequal subset|exact]

Semantics, in full (tests/_swd_ref.py restates them in numpy).  All pyramid arithmetic in float64, every operation rounded on its own.

Input.  (N, 3, H, W), float32, bfloat16 or uint8, any strides.  A value is widened and mapped ``v * scale + shift`` with
``wu.paired.range_mapping(value_range)``.

Filter.  ``f = (1, 4, 6, 4, 1) / 16``.  The blur ``B(g)`` is separable, along H first and then along W, taps in ascending order
(``a = f[0] v[0]; a = a + f[t] v[t]``), the border mirrored without repeating the edge sample: index ``i < 0 -> -i``,
``i >= n -> 2 (n - 1) - i`` (scipy's ``mode='mirror'``, numpy's ``reflect``).

Pyramid.  ``G_0`` is the mapped input; ``G_{l+1}[y, x] = B(G_l)[2y, 2x]``; ``Z[2y, 2x] = G_{l+1}[y, x]``, 0 elsewhere, of size 2h x 2w;
``U_l`` is the same separable pass over ``Z`` with taps ``2 f``, same mirror rule and tap order; ``L_l = G_l - U_l`` for l < levels - 1 and
``L_{levels-1} = G_{levels-1}``.

Levels.  The default is the number of r in ``min(H, W), min(H, W) // 2, ...`` with r >= 16 (``default_levels``: 5 at 256, 4 at 224, 6 at
512).  ``check_levels`` raises -- nothing is ever cropped or padded -- when H or W is not divisible by ``2^(levels-1)``, when a level is
smaller than 7 in either dimension, or when ``levels < 1``.

Descriptors.  P per image and level (128 by default).  Descriptor (n, p) of level l is the 3 x 7 x 7 neighbourhood of ``L_l[n]`` centred at
``positions[l, n, p] = (cy, cx)`` with ``3 <= cy <= H_l - 4`` and ``3 <= cx <= W_l - 4``, flattened as ``c * 49 + dy * 7 + dx`` and rounded
to float32.  Positions come from the host.

Normalisation.  Per level and per set, over all ``m = N P`` descriptors: for channel c, ``mu_c`` and ``sigma_c`` are the mean and the
population standard deviation of its 49 m float32 values, accumulated in float64; the value becomes ``float32((double(v) - mu_c) /
sigma_c)``.  Where ``sigma_c == 0`` the channel's values become 0 -- a departure from PGGAN, which divides by zero there.

Draws (``draw``).  ``rng = np.random.RandomState(seed)``.  First the directions: ``rng.randn(147, ndirs)``, columns normalised to unit
length in float64, ``.astype(float32)``; they are returned transposed, (ndirs, 147), one direction per row.  Then the positions, image by
image: for image i = 0, 1, .. and, inside it, level l = 0 .. levels - 1, ``cy = rng.randint(3, H_l - 3, size=P)`` and then
``cx = rng.randint(3, W_l - 3, size=P)``.  Image i's positions therefore do not depend on how many images follow it; ``first=k`` returns the
positions of images k .. k + n - 1 of that one sequence, which is how ``wu.evaluate.SlicedWasserstein`` makes two batches equal one call.
Both sets of a comparison use the same positions and directions.

Distance.  For direction j: ``a = sort(D1 @ dir_j)``, ``b = sort(D2 @ dir_j)``, products and sums in float64 on the float32 operands;
``w_j = mean_i |a_i - b_i|``; the level's SWD is ``mean_j w_j``.  ``swd`` reports it times 1e3, as PGGAN's tables do, and the mean over
levels.  Inputs must be finite.  ``m1 != m2`` raises unless ``unequal="exact"`` is given; then ``w_j`` is the exact W1 of the two empirical
distributions, ``integral over t in [0, 1] of |Fa^-1(t) - Fb^-1(t)|``, by this rule.  Let x be the longer sorted column (``ml`` keys) and
y the shorter (``ms <= ml``), and measure t in units of ``1 / (ml ms)``: ``x_i`` owns ``[i ms, (i + 1) ms)`` and ``y_j`` owns
``[j ml, (j + 1) ml)``, and an interval of length ``ms <= ml`` meets at most two of y's.  In int64: ``lo = i ms``, ``hi = lo + ms``,
``j0 = lo // ml``, ``j1 = (hi - 1) // ml`` (``j0`` or ``j0 + 1``), ``cut = (j0 + 1) ml``, ``w0 = min(hi, cut) - lo``,
``w1 = hi - min(hi, cut)`` (0 exactly when ``j1 == j0``), and ``w_j = (sum_i w0 |x_i - y_j0| + w1 |x_i - y_j1|) / (ml ms)`` with the
weights converted to float64 (exact) and every product and sum rounded on its own.  No approximation and no search; which set is called a
or b changes no bit.  Equal counts with ``unequal="exact"`` take the equal-count path and give today's bits (the rule reduces to
``mean_i |a_i - b_i|`` there).  ``swd(..., unequal="exact")`` takes sets of ``Na`` and ``Nb`` images of one size: positions are one
``draw`` over ``max(Na, Nb)`` images and image i of either set gets the positions of image i.  ``DescriptorBank`` keeps the raw
descriptors of a stream of batches (or of a directory, ``from_dir``) and ``compare(bank_a, bank_b)`` is the same number for two banks of
any two counts; ``wu.evaluate.SlicedWasserstein(reference=bank)`` compares the outputs with such a bank instead of the input batch.

Kernels (csrc/swd.hip): the pyramid keeps only G_1.. in float64 (a third of the input), forms L_l at the gathered pixels only, projects in
64 x 64 tiles on the fp64 matrix cores, sorts every (direction, set) column with an on-chip bitonic block sort and global merge passes, and
sums in fixed orders: no atomics, two runs give the same bits, and ``dir_chunk`` (how many directions are in flight) changes the memory
in use and nothing else.  CUDA tensors only: there is no CPU fallback."""
import collections

import numpy as np
import torch

from . import _lib
from .layout import stream_ptr
from .paired import U8, range_mapping

D = 147
PATCH = 7
MIN_SIZE = 16                           # the smallest resolution that still gets a default level
MAX_M, MAX_DIRS = 1 << 21, 4096
PAIR_BYTES = 1 << 30                    # sliced_wasserstein keeps at most this many bytes of sorted columns (both sets) alive at once
_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: U8}

SWDResult = collections.namedtuple("SWDResult", "levels mean")


def default_levels(h, w):
    """The number of r in min(h, w), min(h, w) // 2, ... with r >= 16."""
    r, n = min(int(h), int(w)), 0
    while r >= MIN_SIZE:
        n += 1
        r //= 2
    return n


def check_levels(h, w, levels):
    """ValueError unless a pyramid of ``levels`` levels exists for h x w without cropping or padding; returns [(H_l, W_l)]."""
    h, w, levels = int(h), int(w), int(levels)
    if levels < 1:
        raise ValueError(f"swd: levels {levels} must be at least 1 (an image of {h} x {w} has {default_levels(h, w)} by default)")
    step = 1 << (levels - 1)
    if h % step or w % step:
        raise ValueError(f"swd: {h} x {w} is not divisible by 2^(levels-1) = {step}; resize first, nothing is cropped or padded")
    if h // step < PATCH or w // step < PATCH:
        raise ValueError(f"swd: level {levels - 1} of {h} x {w} is {h // step} x {w // step}, smaller than the {PATCH} x {PATCH} patch")
    return [(h >> l, w >> l) for l in range(levels)]


def draw(seed, levels, shapes, n, P, ndirs, first=0):
    """(positions, dirs): int32 (levels, n, P, 2) centres (cy, cx) and float32 (ndirs, 147) unit directions, in the order the module
    docstring fixes.  shapes: [(H_l, W_l)] per level."""
    if len(shapes) != levels or n < 1 or P < 1 or ndirs < 1 or first < 0:
        raise ValueError(f"draw: {len(shapes)} shapes for {levels} levels, n {n}, P {P}, ndirs {ndirs}, first {first}")
    rng = np.random.RandomState(seed)
    d = rng.randn(D, ndirs)
    d = d / np.sqrt(np.sum(np.square(d), axis=0, keepdims=True))
    dirs = np.ascontiguousarray(d.astype(np.float32).T)
    pos = np.empty((levels, n, P, 2), dtype=np.int32)
    for i in range(first + n):
        for l, (hl, wl) in enumerate(shapes):
            cy = rng.randint(3, hl - 3, size=P)
            cx = rng.randint(3, wl - 3, size=P)
            if i >= first:
                pos[l, i - first, :, 0] = cy
                pos[l, i - first, :, 1] = cx
    return pos, dirs


def _require_cuda(*tensors):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError("wu.swd: CUDA tensors only -- no CPU fallback")


def descriptors(images, positions, value_range=(-1, 1), levels=None):
    """The raw descriptors of every level: a list of (N * P, 147) float32 CUDA tensors (views of one buffer).  images (N, 3, H, W) float32,
    bfloat16 or uint8, any strides; positions (levels, N, P, 2) as ``draw`` returns them (numpy or tensor)."""
    _require_cuda(images)
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"descriptors: images must be (N, 3, H, W), got {tuple(images.shape)}")
    if images.dtype not in _DTYPES:
        raise ValueError(f"descriptors: float32, bfloat16 or uint8, got {images.dtype}")
    n, _, h, w = images.shape
    if levels is None:
        levels = default_levels(h, w)
    shapes = check_levels(h, w, levels)
    pos = positions.cpu().numpy() if torch.is_tensor(positions) else np.asarray(positions)
    if pos.ndim != 4 or pos.shape[0] != levels or pos.shape[1] != n or pos.shape[3] != 2 or pos.shape[2] < 1:
        raise ValueError(f"descriptors: positions must be (levels {levels}, N {n}, P, 2), got {pos.shape}")
    P = pos.shape[2]
    for l, (hl, wl) in enumerate(shapes):
        cy, cx = pos[l, :, :, 0], pos[l, :, :, 1]
        if cy.min() < 3 or cy.max() > hl - 4 or cx.min() < 3 or cx.max() > wl - 4:
            raise ValueError(f"descriptors: a position of level {l} ({hl} x {wl}) leaves 3 <= cy <= {hl - 4}, 3 <= cx <= {wl - 4}")
    scale, shift, _ = range_mapping(value_range)
    images = images.detach()
    lib = _lib.load()
    dev = images.device
    nbytes = lib.wu_swd_pyramid_workspace_bytes(n, h, w, levels, P)
    if nbytes == 0:
        raise ValueError(f"descriptors: N {n} P {P} H {h} W {w} levels {levels} out of the kernel's range (N P <= {MAX_M})")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pos_d = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int32)).to(dev)
    out = torch.empty(levels, n * P, D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wu_swd_descriptors", images.data_ptr(), *images.stride(), _DTYPES[images.dtype], n, h, w, scale, shift, levels,
                  pos_d.data_ptr(), P, ws.data_ptr(), out.data_ptr(), stream_ptr())
    return [out[l] for l in range(levels)]


def _rows(desc, what):
    _require_cuda(desc)
    if desc.dim() != 2 or desc.shape[1] != D or desc.dtype != torch.float32:
        raise ValueError(f"{what}: (m, 147) float32 descriptors, got {tuple(desc.shape)} {desc.dtype}")
    return desc.detach().contiguous()


def normalize(desc):
    """(desc_n, mu, sigma): the descriptors of one level and one set normalised per channel, and the three means and three population
    standard deviations as float64 CUDA tensors."""
    desc = _rows(desc, "normalize")
    m = desc.shape[0]
    lib = _lib.load()
    nbytes = lib.wu_swd_stats_workspace_bytes(m)
    if nbytes == 0:
        raise ValueError(f"normalize: m {m} out of the kernel's range 1..{MAX_M}")
    dev = desc.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty_like(desc)
    stats = torch.empty(6, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wu_swd_normalize", desc.data_ptr(), m, ws.data_ptr(), out.data_ptr(), stats.data_ptr(), stream_ptr())
    return out, stats[:3], stats[3:]


def sorted_projections(desc, dirs, dir_chunk=0):
    """(ndirs, m) float64 CUDA: row j is the ascending sort of ``desc @ dirs[j]``."""
    desc, dirs = _rows(desc, "sorted_projections"), _rows(dirs, "sorted_projections")
    m, nd = desc.shape[0], dirs.shape[0]
    lib = _lib.load()
    nbytes = lib.wu_swd_workspace_bytes(m, nd, int(dir_chunk))
    if nbytes == 0:
        raise ValueError(f"sorted_projections: m {m} (1..{MAX_M}), ndirs {nd} (1..{MAX_DIRS}) or dir_chunk {dir_chunk} out of range")
    dev = desc.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(nd, m, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wu_swd_project_sort", desc.data_ptr(), m, dirs.data_ptr(), nd, int(dir_chunk), ws.data_ptr(), out.data_ptr(), stream_ptr())
    return out


def sort_columns(keys):
    """The segmented sort on its own: every row of the contiguous (ncols, m) float64 CUDA tensor ``keys`` ascending, IN PLACE; returns it."""
    _require_cuda(keys)
    if keys.dim() != 2 or keys.dtype != torch.float64 or not keys.is_contiguous():
        raise ValueError(f"sort_columns: a contiguous (ncols, m) float64 tensor, got {tuple(keys.shape)} {keys.dtype}")
    nc, m = keys.shape
    nbytes = _lib.load().wu_swd_workspace_bytes(m, nc, nc)
    if nbytes == 0:
        raise ValueError(f"sort_columns: m {m} (1..{MAX_M}) or ncols {nc} (1..{MAX_DIRS}) out of range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    with torch.cuda.device(keys.device):
        _lib.call("wu_swd_sort_columns", keys.data_ptr(), m, nc, ws.data_ptr(), stream_ptr())
    return keys


def _check_unequal(unequal, what):
    if unequal not in ("raise", "exact"):
        raise ValueError(f"{what}: unequal must be \"raise\" or \"exact\", got {unequal!r}")


def _one_against_rows(d1, rows, dirs, dir_chunk, what, unequal="exact"):
    """One (ndirs,) float64 CUDA tensor per element of ``rows``: ``d1`` (m1, 147) against each (m_r, 147) of ``rows``, all normalised
    float32 descriptors of any counts.  A direction group holds ``PAIR_BYTES // (8 * (m1 + max m_r))`` directions; the columns of ``d1``
    are sorted once per group, whatever the number of rows.  Equal counts go through wu_swd_distance, the others through
    wu_swd_distance_unequal."""
    if not torch.is_tensor(dirs):
        _require_cuda(d1, *rows)
        dirs = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32)).to(d1.device)
    d1, rows, dirs = _rows(d1, what), [_rows(r, what) for r in rows], _rows(dirs, what)
    m1, nd = d1.shape[0], dirs.shape[0]
    sizes = [m1] + [r.shape[0] for r in rows]
    if unequal == "raise" and max(sizes) != min(sizes):
        raise ValueError(f"{what}: {m1} descriptors against {[m for m in sizes[1:] if m != m1][0]}; unequal counts are not supported")
    if not (1 <= min(sizes) and max(sizes) <= MAX_M and 1 <= nd <= MAX_DIRS) or dir_chunk < 0:
        raise ValueError(f"{what}: m {sizes} (1..{MAX_M}), ndirs {nd} (1..{MAX_DIRS}) or dir_chunk {dir_chunk} out of range")
    group = max(1, min(nd, PAIR_BYTES // (8 * (m1 + max(sizes[1:])))))
    out = [torch.empty(nd, dtype=torch.float64, device=d1.device) for _ in rows]
    with torch.cuda.device(d1.device):
        for j0 in range(0, nd, group):
            a = sorted_projections(d1, dirs[j0:j0 + group], dir_chunk)
            for d2, w in zip(rows, out):
                b = sorted_projections(d2, dirs[j0:j0 + group], dir_chunk)
                if d2.shape[0] == m1:
                    _lib.call("wu_swd_distance", a.data_ptr(), b.data_ptr(), m1, a.shape[0], w[j0:].data_ptr(), stream_ptr())
                else:
                    _lib.call("wu_swd_distance_unequal", a.data_ptr(), m1, b.data_ptr(), d2.shape[0], a.shape[0], w[j0:].data_ptr(),
                              stream_ptr())
    return out


def sliced_wasserstein(d1, d2, dirs, dir_chunk=0, unequal="raise"):
    """(ndirs,) float64 CUDA: ``w_j = mean_i |sort(d1 @ dir_j)_i - sort(d2 @ dir_j)_i|``.  d1, d2 (m, 147) float32 normalised descriptors,
    dirs (ndirs, 147) float32 (numpy or CUDA).  Directions go through in groups, so the sorted columns of both sets never take more than
    about ``PAIR_BYTES``; inside a group the library handles ``dir_chunk`` directions per pass (0: its own choice).  Neither changes a bit
    of the result.  ``unequal="exact"``: d1 (m1, 147) and d2 (m2, 147) of any two counts, ``w_j`` the exact W1 of the two sorted columns
    (the module docstring's rule); equal counts give the same bits as the default."""
    _check_unequal(unequal, "sliced_wasserstein")
    return _one_against_rows(d1, [d2], dirs, dir_chunk, "sliced_wasserstein", unequal)[0]


def report(level_values):
    """SWDResult of the per-level distances (any iterable of numbers): each times 1e3, and their mean."""
    lv = tuple(float(v) * 1e3 for v in level_values)
    return SWDResult(lv, float(np.mean(lv)))


def distances(desc_a, desc_b, dirs, dir_chunk=0, unequal="raise"):
    """Per level: normalise both sets' raw descriptors, project, sort, and take the mean over directions -> (levels,) float64 CUDA.
    ``unequal="exact"``: the two sets may hold different numbers of descriptors."""
    _check_unequal(unequal, "distances")
    out = []
    for da, db in zip(desc_a, desc_b):
        out.append(sliced_wasserstein(normalize(da)[0], normalize(db)[0], dirs, dir_chunk, unequal).mean())
    return torch.stack(out)


def distances_to_rows(desc_ref, desc_rows, dirs, dir_chunk=0):
    """``distances(desc_ref, desc_rows[r], ..., unequal="exact")`` for every r, stacked to (R, levels) float64 CUDA, the same bits: per
    level the reference set is normalised once and each of its direction groups sorted once, whatever R."""
    out = []
    for l, ref in enumerate(desc_ref):
        ws = _one_against_rows(normalize(ref)[0], [normalize(row[l])[0] for row in desc_rows], dirs, dir_chunk, "distances_to_rows")
        out.append(torch.stack([w.mean() for w in ws]))
    return torch.stack(out, 1)


def swd(images_a, images_b, P=128, repeats=4, dirs_per_repeat=128, seed=0, value_range=(-1, 1), levels=None, dir_chunk=0, unequal="raise"):
    """SWDResult(levels, mean): the sliced Wasserstein distance x 1e3 of two image sets of one size and count, per pyramid level (finest
    first) and averaged.  Both sets use the same positions and the same ``repeats * dirs_per_repeat`` directions, drawn from ``seed``.
    ``unequal="exact"``: (Na, 3, H, W) against (Nb, 3, H, W); the positions are one ``draw`` over max(Na, Nb) images, image i of either set
    gets those of image i, and every direction's distance is the exact W1 of the two unequal samples."""
    _check_unequal(unequal, "swd")
    _require_cuda(images_a, images_b)
    if unequal == "raise":
        if images_a.dim() != 4 or tuple(images_a.shape) != tuple(images_b.shape):
            raise ValueError(f"swd: two sets of one shape (N, 3, H, W), got {tuple(images_a.shape)} / {tuple(images_b.shape)}; unequal "
                             "counts are not supported")
    elif images_a.dim() != 4 or images_b.dim() != 4 or tuple(images_a.shape[1:]) != tuple(images_b.shape[1:]):
        raise ValueError(f"swd: two sets (Na, 3, H, W) and (Nb, 3, H, W) of one image size, got {tuple(images_a.shape)} / "
                         f"{tuple(images_b.shape)}")
    na, nb = images_a.shape[0], images_b.shape[0]
    _, _, h, w = images_a.shape
    if levels is None:
        levels = default_levels(h, w)
    shapes = check_levels(h, w, levels)
    pos, dirs = draw(seed, levels, shapes, max(na, nb), int(P), int(repeats) * int(dirs_per_repeat))
    da = descriptors(images_a, pos[:, :na], value_range, levels)
    db = descriptors(images_b, pos[:, :nb], value_range, levels)
    return report(distances(da, db, dirs, dir_chunk, unequal).tolist())


# ----------------------------------------------------------------------------------------------
# descriptor banks: sets of any two counts
# ----------------------------------------------------------------------------------------------
class DescriptorBank:
    """The raw per-level descriptors of a stream of image batches, kept on the device (75 KB per image and level at P = 128): one side of
    ``compare``, or the ``reference=`` of ``wu.evaluate.SlicedWasserstein``.  ``add(images)``: (B, 3, H, W) float32, bfloat16 or uint8
    CUDA, one image size for the whole stream; image i of the stream gets the positions ``draw`` gives image i, so any split into batches
    equals one call, bit for bit, and two banks of one ``signature()`` have used the same positions for their common images."""

    def __init__(self, P=128, repeats=4, dirs_per_repeat=128, seed=0, value_range=(-1, 1), levels=None):
        self.P, self.ndirs, self.seed = int(P), int(repeats) * int(dirs_per_repeat), seed
        self.value_range, self.levels = value_range, levels
        self.count, self.shape, self.mapping, self.parts = 0, None, None, []

    @torch.no_grad()
    def add(self, images):
        _require_cuda(images)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"DescriptorBank.add: images must be (B, 3, H, W), got {tuple(images.shape)}")
        b, _, h, w = images.shape
        mapping = tuple(range_mapping(self.value_range)[:2])
        if self.shape is None:
            self.shape, self.mapping = (h, w), mapping
            if self.levels is None:
                self.levels = default_levels(h, w)
        elif self.shape != (h, w) or self.mapping != mapping:
            raise ValueError(f"DescriptorBank.add: {h} x {w} mapped {mapping} after {self.shape[0]} x {self.shape[1]} mapped {self.mapping}")
        shapes = check_levels(h, w, self.levels)
        pos, _ = draw(self.seed, self.levels, shapes, b, self.P, self.ndirs, first=self.count)
        self.parts.append(descriptors(images, pos, self.value_range, self.levels))
        self.count += b
        return self

    def signature(self):
        """What two banks must share to be compared: P, seed, ndirs, levels, the image size and the (scale, shift) of the value range."""
        if not self.parts:
            raise RuntimeError("DescriptorBank: no batch has been added yet")
        return {"P": self.P, "seed": self.seed, "ndirs": self.ndirs, "levels": self.levels, "image size": self.shape,
                "value-range mapping": self.mapping}

    def descriptors(self):
        """[(count * P, 147) float32 CUDA per level]; the batches are joined once and kept joined."""
        self.signature()
        if len(self.parts) > 1:
            self.parts = [[torch.cat([part[l] for part in self.parts]) for l in range(self.levels)]]
        return self.parts[0]

    def directions(self):
        """The (ndirs, 147) float32 directions of ``draw`` for this bank's seed."""
        return draw(self.seed, self.levels, check_levels(*self.shape, self.levels), 1, 1, self.ndirs)[1]

    @classmethod
    def from_dir(cls, dir, size=None, filter=None, gpu_decode=False, device="cuda:0", batch_size=64, **kwargs):
        """The bank of every .jpg / .png file of ``dir`` in sorted order, read through ``wu.files.read_images`` (``size``, ``filter``,
        ``gpu_decode`` as there); ``kwargs`` go to the constructor.  The value range is the reader's."""
        from .files import image_files, read_images
        files = image_files(dir)
        if not files:
            raise RuntimeError(f"no .jpg / .png images in {dir}")
        bank = cls(**kwargs)
        for x, value_range in read_images(files, size, gpu_decode, device, batch_size, filter=filter):
            bank.value_range = value_range
            bank.add(x)
        return bank


def check_comparable(sig_a, sig_b, what):
    """ValueError naming the entries in which two ``DescriptorBank.signature()`` dictionaries differ."""
    differ = [f"{k} {sig_a[k]} / {sig_b[k]}" for k in sig_a if sig_a[k] != sig_b[k]]
    if differ:
        raise ValueError(f"{what}: the two sides must share P, seed, ndirs, levels, image size and value-range mapping; they differ in "
                         + ", ".join(differ))


def compare(bank_a, bank_b, dir_chunk=0):
    """SWDResult of two ``DescriptorBank``s of any two image counts: per level and direction the exact W1 of the two samples (equal counts:
    the bits of ``swd`` on the same images).  ValueError unless the banks share ``signature()``."""
    check_comparable(bank_a.signature(), bank_b.signature(), "compare")
    return report(distances_to_rows(bank_a.descriptors(), [bank_b.descriptors()], bank_a.directions(), dir_chunk)[0].tolist())


# ----------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------
def swd_of_dirs(dir_a, dir_b, size=None, P=128, repeats=4, dirs_per_repeat=128, seed=0, gpu_decode=False, device="cuda:0", log=print,
                filter=None, unequal="subset"):
    """SWDResult of the .jpg / .png files of two directories, and the number of images used per set.  Images are resized (through
    ``wu.input_pipeline``) only with ``size``; otherwise mixed sizes are an error.  Directories of unequal count: a random subset of the
    larger one, drawn from ``seed``, and a line through ``log`` that says so.  ``filter`` (box, bilinear, bicubic, lanczos; with ``size``):
    resize with that Pillow filter in 8-bit mode through ``wu.resample`` instead.  ``unequal="exact"``: every image of both directories
    (``compare`` of two ``DescriptorBank.from_dir``); the second value is then the pair (images of dir_a, images of dir_b)."""
    from .evaluate import SlicedWasserstein
    from .files import image_files, read_images
    if unequal not in ("subset", "exact"):
        raise ValueError(f"swd_of_dirs: unequal must be \"subset\" or \"exact\", got {unequal!r}")
    fa, fb = image_files(dir_a), image_files(dir_b)
    if not fa or not fb:
        raise RuntimeError(f"no .jpg / .png images in {dir_a if not fa else dir_b}")
    if unequal == "exact":
        banks = [DescriptorBank.from_dir(d, size, filter, gpu_decode, device, P=P, repeats=repeats, dirs_per_repeat=dirs_per_repeat, seed=seed)
                 for d in (dir_a, dir_b)]
        return compare(*banks), (banks[0].count, banks[1].count)
    n = min(len(fa), len(fb))
    if len(fa) != len(fb):
        big = fa if len(fa) > n else fb
        keep = sorted(np.random.RandomState(seed).permutation(len(big))[:n].tolist())
        log(f"{dir_a} holds {len(fa)} images and {dir_b} {len(fb)}: using a random subset (seed {seed}) of {n} of the larger set, "
            f"{n} images per set")
        if big is fa:
            fa = [fa[i] for i in keep]
        else:
            fb = [fb[i] for i in keep]
    acc = SlicedWasserstein(P=P, repeats=repeats, dirs_per_repeat=dirs_per_repeat, seed=seed)
    for (xa, ra), (xb, rb) in zip(read_images(fa, size, gpu_decode, device, filter=filter),
                                      read_images(fb, size, gpu_decode, device, filter=filter)):
        acc.value_range = ra
        acc.update(xa, xb)
    return acc.compute(), n


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wu.swd", description="sliced Wasserstein distance on Laplacian-pyramid patches of two "
                                 "directories of images (x 1e3, per pyramid level and averaged)")
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--size", type=int, default=None, help="resize every image to SIZE x SIZE first (otherwise all must have one size)")
    ap.add_argument("--patches", type=int, default=128, help="descriptors per image and level")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--dirs", type=int, default=128, help="directions per repeat")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gpu-decode", action="store_true", help="read the JPEG files through wu.jpeg.GPUJpegDecoder")
    ap.add_argument("--filter", default=None, choices=["box", "bilinear", "bicubic", "lanczos"],
                    help="with --size: resize with this Pillow filter (Image.resize, 8-bit) through wu.resample; absent: the training "
                         "pipeline's bilinear resize, as before")
    ap.add_argument("--unequal", default="subset", choices=["subset", "exact"],
                    help="directories of unequal count: subset (default) compares a seeded random subset of the larger one; exact uses "
                         "every image of both and takes the exact W1 of the unequal samples per direction")
    args = ap.parse_args(argv)
    if args.filter is not None and not args.size:
        ap.error("--filter chooses how --size resizes: give --size")
    r, n = swd_of_dirs(args.dir_a, args.dir_b, args.size, args.patches, args.repeats, args.dirs, args.seed, args.gpu_decode, filter=args.filter,
                       unequal=args.unequal)
    for l, v in enumerate(r.levels):
        print(f"SWD x 1e3, level {l}: {v:.4f}")
    print(f"SWD x 1e3, mean: {r.mean:.4f}")
    print(f"images: {n[0]} against {n[1]}" if args.unequal == "exact" else f"images per set: {n}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
