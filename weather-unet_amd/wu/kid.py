"""Kernel Inception Distance (Binkowski et al. 2018) on the pool3 features of the HIP InceptionV3: the unbiased polynomial-kernel MMD^2,
averaged over random subsets.  Unlike the FID it needs no D x D covariance, so it is usable on a few hundred images (the 500-photograph
test split), where the Frechet distance runs on a rank-deficient matrix.

    bank1, bank2 = FeatureBank(), FeatureBank()          # wu.features.FeatureBank, importable from here too
    bank1.append(feats)                               # (B, D) float32 CUDA rows, what FIDStatistics.update_features takes
    mean, std = kernel_inception_distance(bank1, bank2)  # 100 subsets of 1000 rows, k(x, y) = (<x, y> / D + 1)^3

Semantics, in full.  ``rng = np.random.RandomState(seed)``; for every subset, ``rng.choice(n1, m, replace=False)`` and then
``rng.choice(n2, m, replace=False)``.  ``k(x, y) = (gamma <x, y> + coef0)^degree`` in float64 on the float32 rows (gamma None = 1 / D).
Per subset ``sxx = sum_{i != j} k(x_i, x_j)``, ``syy`` likewise, ``sxy = sum_{i, j} k(x_i, y_j)`` and
``mmd2 = (sxx + syy) / (m (m - 1)) - 2 sxy / (m m)``; the result is ``(np.mean, np.std)`` of the subsets' mmd2.  A subset size over
min(n1, n2) is an error, never clamped.

All subsets run in two launches (wu_kid_mmd, csrc/kid.hip on the fp64 tile of csrc/gram_f64.h): the rows are gathered through the index
array on the device and the kernel matrices are never stored.  There is no host fallback."""
import numpy as np
import torch

from . import _lib
from .features import FeatureBank, as_rows  # noqa: F401  (wu.kid.FeatureBank is the documented name of the class)
from .layout import stream_ptr


def _check_subset_size(n1, n2, m):
    if m < 2 or m > min(n1, n2):
        raise ValueError(f"KID: subset_size m = {m} must be at least 2 and at most min(n1 = {n1}, n2 = {n2}); lower subset_size "
                         f"(it is never clamped silently)")


def subset_indices(n1, n2, num_subsets, subset_size, seed):
    """(S, 2, m) int32: per subset the m rows of the first bank, then the m of the second, each drawn without replacement from one
    ``np.random.RandomState(seed)`` in that order."""
    _check_subset_size(n1, n2, subset_size)
    if num_subsets < 1:
        raise ValueError(f"KID: num_subsets {num_subsets} must be at least 1")
    rng = np.random.RandomState(seed)
    out = np.empty((num_subsets, 2, subset_size), dtype=np.int32)
    for s in range(num_subsets):
        out[s, 0] = rng.choice(n1, subset_size, replace=False)
        out[s, 1] = rng.choice(n2, subset_size, replace=False)
    return out


def polynomial_mmd_subsets(f1, f2, indices, degree=3, gamma=None, coef0=1.0):
    """The thin wrapper over wu_kid_mmd.  f1 (n1, D), f2 (n2, D): float32 CUDA rows with unit column stride (any row stride);
    indices: (S, 2, m) integers (numpy or tensor), [:, 0] into f1 and [:, 1] into f2, checked here on the host.  Returns
    (sums (S, 3) = (sxx, syy, sxy), mmd2 (S,)) as float64 CUDA tensors; nothing is synchronised."""
    f1, f2 = as_rows(f1, "polynomial_mmd_subsets"), as_rows(f2, "polynomial_mmd_subsets")
    if f1.shape[1] != f2.shape[1] or f1.device != f2.device:
        raise ValueError(f"polynomial_mmd_subsets: feature widths {f1.shape[1]} / {f2.shape[1]} or devices differ")
    idx = indices.detach().cpu().numpy() if torch.is_tensor(indices) else np.asarray(indices)
    if idx.ndim != 3 or idx.shape[1] != 2 or idx.dtype.kind not in "iu":
        raise ValueError(f"polynomial_mmd_subsets: indices must be an integer array of shape (S, 2, m), got {idx.dtype} {idx.shape}")
    (n1, d), n2 = f1.shape, f2.shape[0]
    s, _, m = idx.shape
    if s < 1 or s > 65535:
        raise ValueError(f"polynomial_mmd_subsets: {s} subsets outside 1..65535")
    _check_subset_size(n1, n2, m)
    if int(degree) != degree or degree < 1:
        raise ValueError(f"polynomial_mmd_subsets: degree {degree} must be an integer >= 1")
    if idx[:, 0].min() < 0 or idx[:, 0].max() >= n1 or idx[:, 1].min() < 0 or idx[:, 1].max() >= n2:
        raise ValueError(f"polynomial_mmd_subsets: an index lies outside its bank (n1 = {n1}, n2 = {n2})")
    if gamma is None:
        gamma = 1.0 / d
    lib = _lib.load()
    dev = f1.device
    idx_dev = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    ws = torch.empty(lib.wu_kid_workspace_bytes(s, m), dtype=torch.uint8, device=dev)
    sums = torch.empty(s, 3, dtype=torch.float64, device=dev)
    mmd2 = torch.empty(s, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("wu_kid_mmd", f1.data_ptr(), f1.stride(0), n1, f2.data_ptr(), f2.stride(0), n2, idx_dev.data_ptr(), s, m, d, int(degree),
                  float(gamma), float(coef0), ws.data_ptr(), sums.data_ptr(), mmd2.data_ptr(), stream_ptr())
    return sums, mmd2


def kernel_inception_distance(f1, f2, num_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=2020):
    """(mean, std) of the unbiased polynomial MMD^2 over ``num_subsets`` random subsets of ``subset_size`` rows of f1 and f2 (FeatureBanks
    or (n, D) float32 CUDA tensors).  ValueError when subset_size exceeds min(n1, n2)."""
    f1, f2 = as_rows(f1, "kernel_inception_distance"), as_rows(f2, "kernel_inception_distance")
    idx = subset_indices(f1.shape[0], f2.shape[0], num_subsets, subset_size, seed)
    _, mmd2 = polynomial_mmd_subsets(f1, f2, idx, degree, gamma, coef0)
    v = mmd2.cpu().numpy()
    return float(np.mean(v)), float(np.std(v))
