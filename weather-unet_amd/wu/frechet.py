"""Rank-aware Frechet distance on the feature rows themselves: no covariance, no matrix square root, exact for any rank.

    real, fake = FeatureBank(), FeatureBank()            # wu.features.FeatureBank: the rows --kid / --prdc keep on the GPU
    r = frechet_distance(real, fake)                     # r.fid, r.trace_sqrt, r.mean_term, r.trace1, r.trace2, r.sweeps, r.rotations

With A (n1 x D) and B (n2 x D) the centred rows and Sigma = A^T A / (n - 1) per set, the non-zero eigenvalues of Sigma1 Sigma2 are those of
(A B^T)(A B^T)^T / ((n1 - 1)(n2 - 1)), so

    Tr sqrt(Sigma1 Sigma2) = ||A B^T||_* / sqrt((n1 - 1)(n2 - 1))           (nuclear norm: the sum of the singular values)
    fid = |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 - 2 Tr sqrt(Sigma1 Sigma2)

A B^T is the double-centred cross-Gram matrix of the raw rows, min(n1, n2) x max(n1, n2): 500 x 500 for the 500-photograph test split,
where ``wu.fid.calculate_frechet_distance`` runs scipy's ``sqrtm`` on a 2048 x 2048 product of rank <= 499.  Its singular values come from
a one-sided (Hestenes) Jacobi iteration on the GPU (csrc/frechet.hip; include/wu_kernels.h states every stage): rotations of row pairs in a
round-robin order, one launch per step, until a whole sweep rotates nothing.  The host reads one 4-byte rotation count per sweep.  Every sum
runs in a fixed order, so two runs give the same bits.  There is no host fallback.

Limits: n1, n2 >= 2, equal D, min(n1, n2) <= 4096 (MAX_VECTORS); the work matrix of min(n1, n2) x max(n1, n2) doubles must fit in free
device memory.  Two large sets go through ``wu.fid.calculate_frechet_distance`` on mu / sigma, where the covariances have full rank."""
import collections

import numpy as np
import torch

from . import _lib
from .features import as_rows
from .layout import stream_ptr

MAX_VECTORS = 4096
MAX_ROWS = 1 << 21

FrechetResult = collections.namedtuple(
    "FrechetResult", ["fid", "trace_sqrt", "mean_term", "trace1", "trace2", "sweeps", "rotations", "singular_values"])


def _sweep_until_orthogonal(v, ns, nl, max_sweeps, who):
    """Sweeps over the rows of v (ns x nl float64, unit column stride) until one rotates nothing; the rotation count of every sweep."""
    if int(max_sweeps) != max_sweeps or max_sweeps < 1:
        raise ValueError(f"{who}: max_sweeps = {max_sweeps} must be an integer >= 1")
    counter = torch.empty(1, dtype=torch.int32, device=v.device)
    rotations = []
    while True:
        _lib.call("wu_fd_jacobi_sweep", v.data_ptr(), v.stride(0), ns, nl, counter.data_ptr(), stream_ptr())
        rotations.append(int(counter.item()))            # the one host read per sweep
        if rotations[-1] == 0:
            return rotations
        if len(rotations) >= max_sweeps:
            raise RuntimeError(f"{who}: {rotations[-1]} rotations in sweep {len(rotations)}: the Jacobi iteration has not converged within "
                               f"max_sweeps = {max_sweeps}")


def _finish(v, ns, nl):
    sigma = torch.empty(ns, dtype=torch.float64, device=v.device)
    total = torch.empty(1, dtype=torch.float64, device=v.device)
    _lib.call("wu_fd_finish", v.data_ptr(), v.stride(0), ns, nl, sigma.data_ptr(), total.data_ptr(), stream_ptr())
    return sigma, total


def singular_values(matrix, max_sweeps=60, info=False):
    """The singular values of an (n <= 4096, m) float64 CUDA matrix by the Jacobi stage alone: a float64 CUDA tensor of n values in ROW order,
    not sorted (row i's norm once the rows are orthogonal; with n > m at least n - m of them are 0).  The matrix is not modified.
    ``info=True`` returns (values, their sum in index order as a 1-element tensor, rotations per sweep)."""
    m = matrix
    if not torch.is_tensor(m) or not m.is_cuda or m.dtype != torch.float64 or m.dim() != 2:
        raise ValueError("singular_values: expected an (n, m) float64 CUDA tensor")
    ns, nl = m.shape
    if ns < 1 or ns > MAX_VECTORS or nl < 1 or nl > MAX_ROWS:
        raise ValueError(f"singular_values: shape {tuple(m.shape)} outside (1..{MAX_VECTORS}, 1..{MAX_ROWS})")
    _lib.load()
    with torch.cuda.device(m.device):
        v = m.clone(memory_format=torch.contiguous_format)
        rotations = _sweep_until_orthogonal(v, ns, nl, max_sweeps, "singular_values")
        sigma, total = _finish(v, ns, nl)
    return (sigma, total, rotations) if info else sigma


def _check_pair(real, fake, who):
    x1, x2 = as_rows(real, who), as_rows(fake, who)
    (n1, d), n2 = x1.shape, x2.shape[0]
    if x1.shape[1] != x2.shape[1] or x1.device != x2.device:
        raise ValueError(f"{who}: feature widths {x1.shape[1]} / {x2.shape[1]} or devices differ")
    if d < 1:
        raise ValueError(f"{who}: feature width {d} must be at least 1")
    if n1 < 2 or n2 < 2:
        raise ValueError(f"{who}: n1 = {n1} / n2 = {n2}: a covariance needs at least 2 rows per set")
    if max(n1, n2) > MAX_ROWS:
        raise ValueError(f"{who}: max(n1 = {n1}, n2 = {n2}) over {MAX_ROWS} rows")
    if min(n1, n2) > MAX_VECTORS:
        raise ValueError(f"{who}: min(n1 = {n1}, n2 = {n2}) over {MAX_VECTORS}: the Jacobi iteration rotates the rows of the smaller set; "
                         f"for two large sets use wu.fid.calculate_frechet_distance on mu / sigma")
    return x1, x2


def centred_cross_gram(real, fake):
    """Stages 1 and 2: (V, workspace).  V is the (ns, nl) float64 view (row stride ld) of the double-centred cross-Gram matrix inside the
    workspace tensor, V[i][j] = <a_i, b_j> with a the centred rows of the set with fewer rows (a tie: ``real``).  Nothing is synchronised."""
    x1, x2 = _check_pair(real, fake, "centred_cross_gram")
    (n1, d), n2 = x1.shape, x2.shape[0]
    lib = _lib.load()
    ns, nl = min(n1, n2), max(n1, n2)
    ld, nbytes = lib.wu_fd_ld(n1, n2), lib.wu_fd_workspace_bytes(n1, n2, d)
    if ld == 0 or nbytes == 0:
        raise ValueError(f"centred_cross_gram: n1 = {n1} / n2 = {n2} / D = {d} out of the library's range")
    dev = x1.device
    with torch.cuda.device(dev):
        free, _ = torch.cuda.mem_get_info(dev)
        if nbytes > free:
            raise ValueError(f"centred_cross_gram: the {ns} x {ld} float64 work matrix ({nbytes} bytes) does not fit in the {free} bytes of "
                             f"free device memory; for two large sets use wu.fid.calculate_frechet_distance on mu / sigma")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        _lib.call("wu_fd_cross_gram", x1.data_ptr(), x1.stride(0), n1, x2.data_ptr(), x2.stride(0), n2, d, ws.data_ptr(), stream_ptr())
    return ws[:ns * ld].view(ns, ld)[:, :nl], ws


def moments(rows):
    """Stage 3: (mu (D,), dev2 (n,), s (1,)) float64 CUDA tensors: the mean row, |x_i - mu|^2 per row and their sum; tr Sigma = s / (n - 1)."""
    x = as_rows(rows, "moments")
    n, d = x.shape
    if n < 2 or n > MAX_ROWS or d < 1:
        raise ValueError(f"moments: shape {tuple(x.shape)}: 2 <= n <= {MAX_ROWS} and D >= 1")
    _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        mu = torch.empty(d, dtype=torch.float64, device=dev)
        dev2 = torch.empty(n, dtype=torch.float64, device=dev)
        s = torch.empty(1, dtype=torch.float64, device=dev)
        _lib.call("wu_fd_moments", x.data_ptr(), x.stride(0), n, d, mu.data_ptr(), dev2.data_ptr(), s.data_ptr(), stream_ptr())
    return mu, dev2, s


def frechet_distance(real, fake, max_sweeps=60):
    """The Frechet distance of two FeatureBanks or (n, D) float32 CUDA tensors, as a FrechetResult: ``fid`` and its terms (Python floats:
    fid = ((mean_term + trace1) + trace2) - 2 trace_sqrt), ``sweeps`` and ``rotations`` (per sweep, the last one 0) of the Jacobi iteration,
    and ``singular_values`` of the centred cross-Gram matrix (float64 CUDA tensor, row order).  RuntimeError when ``max_sweeps`` sweeps do
    not converge; ValueError for what the module docstring rules out."""
    x1, x2 = _check_pair(real, fake, "frechet_distance")
    n1, n2 = x1.shape[0], x2.shape[0]
    v, _ws = centred_cross_gram(x1, x2)
    mu1, _, s1 = moments(x1)
    mu2, _, s2 = moments(x2)
    ns, nl = v.shape
    with torch.cuda.device(x1.device):
        rotations = _sweep_until_orthogonal(v, ns, nl, max_sweeps, "frechet_distance")
        sigma, total = _finish(v, ns, nl)
    diff = (mu1 - mu2).cpu().numpy()
    mean_term = float(np.dot(diff, diff))
    trace1, trace2 = float(s1.item()) / float(n1 - 1), float(s2.item()) / float(n2 - 1)
    trace_sqrt = float(float(total.item()) / np.sqrt(float(n1 - 1) * float(n2 - 1)))
    fid = ((mean_term + trace1) + trace2) - 2.0 * trace_sqrt
    return FrechetResult(fid, trace_sqrt, mean_term, trace1, trace2, len(rotations), rotations, sigma)
