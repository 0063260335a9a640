"""Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020, the ``prdc`` package) on the pool3
features of the HIP InceptionV3.  FID, IS and KID each mix fidelity and diversity in one number; these four tell a generator that collapses
towards a prototype (precision and density stay, recall and coverage drop) from one that leaves its input untouched.  Like the KID they need
no covariance, so they are usable on the 500-photograph test split.

    real, fake = FeatureBank(), FeatureBank()                             # wu.features.FeatureBank: rows kept on the GPU
    p, r, d, c = precision_recall_density_coverage(real, fake, k=5)        # prdc's default k; Kynkaanniemi et al. use k = 3

Semantics, in full (prdc's, stated on squared distances).  For float32 rows a, b widened to float64,
``d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0)``, every operation rounded on its own.  ``radius_X[i]`` is the (k + 1)-th smallest of row i
of the n x n matrix d2(x_i, x_j) with the diagonal forced to 0 (the row itself is one of the k + 1, as in prdc and sklearn; duplicate rows
may give radius 0).  With X the real bank (n1 rows) and Y the fake bank (n2 rows), compared with ``<=``:

    A[i] = #{ j : d2(x_i, y_j) <= radius_X[i] }      B[i] = #{ j : d2(x_i, y_j) <= radius_Y[j] }      C[j] = #{ i : d2(x_i, y_j) <= radius_X[i] }
    precision = mean(C > 0)    recall = mean(B > 0)    density = sum(C) / (k n2)    coverage = mean(A > 0)

1 <= k <= 16; a bank with fewer than k + 1 rows is an error, never clamped.

The distance matrices are never stored (wu_knn_radii / wu_prdc_counts, csrc/prdc.hip: 64 x 64 tiles on the fp64 matrix cores, the tile of
csrc/gram_f64.h that the KID shares, consumed by the epilogue).  There is no host fallback."""
import collections

import torch

from . import _lib
from .features import as_rows
from .layout import stream_ptr

MAX_K = 16
MAX_COL_SPLITS = 1024

PRDC = collections.namedtuple("PRDC", ["precision", "recall", "density", "coverage"])


def _rows(f, who):
    f = as_rows(f, who)
    if f.shape[1] < 1:
        raise ValueError(f"{who}: feature width {f.shape[1]} must be at least 1")
    return f


def _check_k(k, col_splits, who):
    if int(k) != k or k < 1 or k > MAX_K:
        raise ValueError(f"{who}: k = {k} must be an integer in 1..{MAX_K}")
    if int(col_splits) != col_splits or col_splits < 0 or col_splits > MAX_COL_SPLITS:
        raise ValueError(f"{who}: col_splits = {col_splits} must be an integer in 0..{MAX_COL_SPLITS} (0: chosen from n)")


def _check_n(n, k, who, name):
    if n < k + 1:
        raise ValueError(f"{who}: the {name} bank has n = {n} rows, k = {k} needs at least k + 1 = {k + 1} (n is never clamped)")


def _workspace(lib, n1, n2, k, col_splits, dev, who):
    nbytes = lib.wu_prdc_workspace_bytes(n1, n2, k, col_splits)
    if nbytes == 0:
        raise ValueError(f"{who}: n1 = {n1} / n2 = {n2} / k = {k} / col_splits = {col_splits} out of the library's range")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _radii(lib, f, k, col_splits, ws):
    n, d = f.shape
    radii = torch.empty(n, dtype=torch.float64, device=f.device)
    _lib.call("wu_knn_radii", f.data_ptr(), f.stride(0), n, d, k, col_splits, ws.data_ptr(), radii.data_ptr(), stream_ptr())
    return radii


def knn_radii(f, k, col_splits=0):
    """(n,) float64 CUDA tensor: per row of f the SQUARED distance to its k-th nearest other row (the (k + 1)-th smallest of the row of the
    n x n matrix with a zero diagonal).  col_splits: 0 lets the library split the columns over workgroups by n; a positive value forces
    that many splits.  Nothing is synchronised."""
    _check_k(k, col_splits, "knn_radii")
    f = _rows(f, "knn_radii")
    k, col_splits = int(k), int(col_splits)
    _check_n(f.shape[0], k, "knn_radii", "only")
    lib = _lib.load()
    with torch.cuda.device(f.device):
        ws = _workspace(lib, f.shape[0], f.shape[0], k, col_splits, f.device, "knn_radii")
        return _radii(lib, f, k, col_splits, ws)


def manifold_counts(real, fake, k, col_splits=0):
    """(A, B, C, radii_real, radii_fake): the three count vectors of the module docstring (A, B of length n1, C of length n2: the library's
    uint32 values in int32 CUDA tensors, a count being at most 2^21) and the two banks' float64 radii.  Nothing is synchronised."""
    _check_k(k, col_splits, "manifold_counts")
    x, y = _rows(real, "manifold_counts"), _rows(fake, "manifold_counts")
    k, col_splits = int(k), int(col_splits)
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise ValueError(f"manifold_counts: feature widths {x.shape[1]} / {y.shape[1]} or devices differ")
    (n1, d), n2 = x.shape, y.shape[0]
    _check_n(n1, k, "manifold_counts", "real")
    _check_n(n2, k, "manifold_counts", "fake")
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        ws = _workspace(lib, n1, n2, k, col_splits, dev, "manifold_counts")
        rx = _radii(lib, x, k, col_splits, ws)
        ry = _radii(lib, y, k, col_splits, ws)
        a = torch.empty(n1, dtype=torch.int32, device=dev)
        b = torch.empty(n1, dtype=torch.int32, device=dev)
        c = torch.empty(n2, dtype=torch.int32, device=dev)
        _lib.call("wu_prdc_counts", x.data_ptr(), x.stride(0), n1, rx.data_ptr(), y.data_ptr(), y.stride(0), n2, ry.data_ptr(), d,
                  ws.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), stream_ptr())
    return a, b, c, rx, ry


def metrics_from_counts(a, b, c, k):
    """The four numbers from the count vectors (tensors or arrays): Python floats, integer sums divided once."""
    a, b, c = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (a, b, c))
    n1, n2 = len(a), len(c)
    return PRDC(precision=int((c > 0).sum()) / n2, recall=int((b > 0).sum()) / n1, density=int(c.sum()) / (k * n2),
                coverage=int((a > 0).sum()) / n1)


def precision_recall_density_coverage(real, fake, k=5):
    """PRDC(precision, recall, density, coverage) of the fake bank against the real one (FeatureBanks or (n, D) float32 CUDA tensors)."""
    a, b, c, _, _ = manifold_counts(real, fake, k)
    return metrics_from_counts(a, b, c, int(k))
