"""The rank-aware Frechet distance on feature rows restated in numpy float64 (what wu.frechet computes through csrc/frechet.hip;
tests/test_frechet_cpu.py and tests/test_gpu_frechet.py), stage by stage, and a one-line np.linalg.svd version as the independent oracle.

Identity.  With A (n1 x D), B (n2 x D) the centred rows and Sigma = A^T A / (n - 1) per set, the non-zero eigenvalues of Sigma1 Sigma2 are
those of (A B^T)(A B^T)^T / ((n1 - 1)(n2 - 1)), so Tr sqrt(Sigma1 Sigma2) = ||A B^T||_* / sqrt((n1 - 1)(n2 - 1)): no covariance and no
matrix square root, exact for any rank.  A B^T is the double-centred cross-Gram matrix of the raw rows.

Orientation.  The "vectors" are the rows of the set with FEWER rows (a tie goes to set 1): V is ns x nl, V[i][j] = <p_i, q_j>.

Order of operations, which the kernels share.  ``block_sum`` is the one reduction of a 256-thread workgroup: thread t adds elements
t, t + 256, .. in that order, the 64 lanes of a wave are folded lane l += lane l + off for off = 32 .. 1, and the four waves are added in
wave order.  Every product and sum is rounded on its own (no fused multiply-add)."""
import numpy as np

U = 2.0 ** -53          # unit roundoff of float64
MAX_VECTORS = 4096


# ---- the fixed-order reductions ----------------------------------------------------------------------------------------------------------
def block_sum(a):
    """The workgroup sum over the last axis of `a` in the kernels' order."""
    a = np.asarray(a, dtype=np.float64)
    L = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (256,), dtype=np.float64)
    for k0 in range(0, L, 256):                          # a thread's elements, in order; a thread past the end adds nothing
        m = min(256, L - k0)
        acc[..., :m] = acc[..., :m] + a[..., k0:k0 + m]
    w = acc.reshape(a.shape[:-1] + (4, 64)).copy()
    for off in (32, 16, 8, 4, 2, 1):                     # wave_sum_f64
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def orient(x1, x2):
    """(p, q, swapped): p the set whose rows are the vectors."""
    return (x1, x2, False) if len(x1) <= len(x2) else (x2, x1, True)


# ---- stage 1 + 2 -----------------------------------------------------------------------------------------------------------------------------
def cross_gram(x1, x2):
    p, q, _ = orient(np.asarray(x1, dtype=np.float32), np.asarray(x2, dtype=np.float32))
    return p.astype(np.float64) @ q.astype(np.float64).T


def centre(V):
    """V[i][j] - r_i / nl - c_j / ns + t / (ns nl), the four terms applied in that order, one rounding per operation.  r_i: block_sum of row
    i; c_j: rows 0, 1, .. added in order; t: block_sum of r."""
    V = np.asarray(V, dtype=np.float64)
    ns, nl = V.shape
    r = block_sum(V)
    c = np.zeros(nl, dtype=np.float64)
    for i in range(ns):
        c = c + V[i]
    t = block_sum(r)
    return ((V - (r / float(nl))[:, None]) - (c / float(ns))[None, :]) + t / (float(ns) * float(nl))


def centred_cross_gram(x1, x2):
    return centre(cross_gram(x1, x2))


# ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------------
def moments(x):
    """(mu (D,), dev2 (n,), s): mu_d = (rows d of the four row groups i = w, w + 4, .. added in order, the groups in order) / n;
    dev2_i = block_sum_d of (x_id - mu_d)^2; s = block_sum of dev2."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, D = x.shape
    part = np.zeros((4, D), dtype=np.float64)
    for i in range(n):
        part[i & 3] = part[i & 3] + x[i]
    mu = (((part[0] + part[1]) + part[2]) + part[3]) / float(n)
    d = x - mu[None, :]
    dev2 = block_sum(d * d)
    return mu, dev2, float(block_sum(dev2))


# ---- stage 4: one-sided (Hestenes) Jacobi ------------------------------------------------------------------------------------------------------
def schedule(ns):
    """The round-robin steps of one sweep: a list of N = 2 ceil(ns / 2) - 1 steps, each a list of ceil(ns / 2) pairs (p, q), p < q.  Step s pairs
    (N, s) and, for k = 1 .. (N - 1) / 2, ((s + k) mod N, (s - k + N) mod N).  A pair with an index >= ns (the phantom of an odd ns) is
    dropped here, as the kernel's workgroup exits."""
    N = 2 * ((ns + 1) // 2) - 1
    steps = []
    for s in range(N):
        pairs = [(N, s)] + [((s + k) % N, (s - k + N) % N) for k in range(1, (N - 1) // 2 + 1)]
        steps.append([(min(a, b), max(a, b)) for a, b in pairs if a < ns and b < ns])
    return steps


def tolerance(nl):
    return np.sqrt(float(nl)) * U          # LAPACK dgesvj's criterion


# A squared norm below DBL_MIN / eps = 2^-969 has lost its relative precision to underflow (its terms are subnormal or gone), so neither the
# threshold nor the rotation can be trusted: such a vector counts as zero and is stored as zero.  Without this a matrix with more vectors than
# length stalls: the surplus vectors shrink sweep by sweep to about 1e-155 and then rotate among themselves for ever on subnormal garbage.
NORM2_FLOOR = 2.0 ** -969


def _dots(a, b, kernel_order):
    return block_sum(a * b) if kernel_order else np.einsum("ij,ij->i", a, b)


def jacobi_step(V, pairs, tol, norm2=None, kernel_order=True):
    """Rotate the (disjoint) row pairs of one step in place; returns the number of rotations.  norm2: the rows' squared norms (block_sum of
    the squares), kept up to date here -- a row that has not changed since has the same sum, so caching it changes no bit.
    kernel_order=False takes the dot products with einsum instead of block_sum: the same schedule, threshold and rotation, several times
    faster on a few hundred vectors, for comparisons that do not depend on the order of summation."""
    if len(pairs) == 0:
        return 0
    pairs = np.asarray(pairs)
    pi, qi = pairs[:, 0], pairs[:, 1]
    if norm2 is None:
        norm2 = _dots(V, V, kernel_order)
    P, Q = V[pi], V[qi]
    alpha, beta, gamma = norm2[pi], norm2[qi], _dots(P, Q, kernel_order)
    with np.errstate(all="ignore"):
        thresh = (tol * np.sqrt(alpha)) * np.sqrt(beta)
        dead_p, dead_q = alpha < NORM2_FLOOR, beta < NORM2_FLOOR
        for idx, dead, a in ((pi, dead_p, alpha), (qi, dead_q, beta)):
            flush = idx[dead & (a != 0.0)]
            V[flush] = 0.0
            norm2[flush] = 0.0
        rot = ~dead_p & ~dead_q & ~(np.abs(gamma) <= thresh)
        k = np.nonzero(rot)[0]
        if len(k) == 0:
            return 0
        alpha, beta, gamma = alpha[k], beta[k], gamma[k]
        zeta = (beta - alpha) / (2.0 * gamma)
        t = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))      # zeta = 0: t = 1
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = c * t
    c, s = c[:, None], s[:, None]
    P, Q = P[k], Q[k]
    newp, newq = c * P - s * Q, s * P + c * Q
    V[pi[k]], V[qi[k]] = newp, newq
    norm2[pi[k]], norm2[qi[k]] = _dots(newp, newp, kernel_order), _dots(newq, newq, kernel_order)
    return len(k)


def jacobi(M, max_sweeps=60, kernel_order=True):
    """(V, rotations per sweep) after sweeping the rows of M until a sweep rotates nothing."""
    V = np.array(M, dtype=np.float64, order="C")
    ns, nl = V.shape
    steps, tol = [np.array(p).reshape(-1, 2) for p in schedule(ns)], tolerance(nl)
    norm2 = _dots(V, V, kernel_order)
    rotations = []
    while True:
        rotations.append(sum(jacobi_step(V, pairs, tol, norm2, kernel_order) for pairs in steps))
        if rotations[-1] == 0:
            return V, rotations
        if len(rotations) >= max_sweeps:
            raise RuntimeError(f"Jacobi: {rotations[-1]} rotations in sweep {len(rotations)}, no convergence in max_sweeps = {max_sweeps}")


# ---- stage 5 -----------------------------------------------------------------------------------------------------------------------------------
def finish(V):
    """(sigma (ns,) in index order, their sum in index order)."""
    sigma = np.sqrt(block_sum(V * V))
    total = 0.0
    for v in sigma:
        total = total + v
    return sigma, float(total)


def singular_values(M, max_sweeps=60, kernel_order=True):
    V, rotations = jacobi(M, max_sweeps, kernel_order)
    return finish(V) + (rotations,)


# ---- the whole ---------------------------------------------------------------------------------------------------------------------------------
def combine(total, n1, n2, s1, s2, mu1, mu2):
    """dict of the terms: trace_sqrt = total / sqrt((n1 - 1)(n2 - 1)), trace_k = s_k / (n_k - 1), mean_term = |mu1 - mu2|^2,
    fid = ((mean_term + trace1) + trace2) - 2 trace_sqrt."""
    trace_sqrt = total / np.sqrt(float(n1 - 1) * float(n2 - 1))
    trace1, trace2 = s1 / float(n1 - 1), s2 / float(n2 - 1)
    d = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    mean_term = float(np.dot(d, d))
    return dict(fid=float(((mean_term + trace1) + trace2) - 2.0 * trace_sqrt), trace_sqrt=float(trace_sqrt), mean_term=float(mean_term),
                trace1=float(trace1), trace2=float(trace2))


def frechet_distance(x1, x2, max_sweeps=60, kernel_order=True):
    x1, x2 = np.asarray(x1, dtype=np.float32), np.asarray(x2, dtype=np.float32)
    sigma, total, rotations = singular_values(centred_cross_gram(x1, x2), max_sweeps, kernel_order)
    mu1, _, s1 = moments(x1)
    mu2, _, s2 = moments(x2)
    out = combine(total, len(x1), len(x2), s1, s2, mu1, mu2)
    out.update(sweeps=len(rotations), rotations=rotations, singular_values=sigma)
    return out


def frechet_distance_svd(x1, x2):
    """The independent oracle: LAPACK's singular values of the centred rows' product."""
    x1, x2 = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (x1, x2))
    a, b = x1 - x1.mean(axis=0), x2 - x2.mean(axis=0)
    nuc = np.linalg.svd(a @ b.T, compute_uv=False).sum()
    d = x1.mean(axis=0) - x2.mean(axis=0)
    return float(d @ d + (a * a).sum() / (len(a) - 1) + (b * b).sum() / (len(b) - 1) - 2 * nuc / np.sqrt((len(a) - 1.0) * (len(b) - 1.0)))


def bound(x1, x2, ref, K):
    """How far two correct evaluations (this file and the device) of frechet_distance may lie apart: a dict with the keys of ``combine``.
    Derived, not tuned; u = 2^-53, features non-negative, g = max_ij <p_i, q_j>, ns <= nl the shape of V.

    trace_sqrt.  (a) Each side's singular values lie within K (ns + nl) u sigma_1 (the device; K = K_GPU) and RECORDED_WORST_RATIO
    (ns + nl) u sigma_1 (this file) of the exact ones of its own matrix: ns (K + RECORDED_WORST_RATIO)(ns + nl) u sigma_1 on their sum.
    (b) The two matrices differ by E, and | ||A||_* - ||B||_* | <= ||E||_* <= sqrt(ns) ||E||_F (Weyl / Mirsky).  Per entry and side:
    the Gram entry (D + 4) u g; the row mean, the column mean and the total mean each that plus (nl + 2) u g, (ns + 2) u g and
    (ns + nl + 3) u g of summing non-negative terms below g and one division; three more roundings of values below 2 g: in all
    e = (4 (D + 4) + 2 (ns + nl) + 13) u g, and ||E||_F <= sqrt(ns nl) 2 e.  Both over sqrt((n1 - 1)(n2 - 1)).

    trace_k = s / (n - 1).  mu_d is a sum of n non-negative terms and a division: dmu = (n + 1) u max|x| per side.  s adds n D terms
    (x - mu)^2: (D + n + 3) u s for the squares and the sums, 2 sum|x - mu| dmu <= 2 sqrt(n D s) dmu for mu's error (Cauchy-Schwarz); twice,
    for the two sides, over n - 1.

    mean_term = sum_d d_d^2, d = mu1 - mu2: dd = 2 (dmu1 + dmu2) + u max|d| per component between the sides, so
    2 sqrt(D mean_term) dd + 2 (D + 2) u mean_term.

    fid: the three bounds, twice that of trace_sqrt, and 3 u (mean_term + trace1 + trace2 + 2 trace_sqrt) for the combination."""
    x1, x2 = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (x1, x2))
    assert x1.min() >= 0 and x2.min() >= 0
    (n1, D), n2 = x1.shape, x2.shape[0]
    ns, nl = min(n1, n2), max(n1, n2)
    g = float((x1 @ x2.T).max())
    sigma1 = float(np.max(ref["singular_values"]))
    a = ns * (K + RECORDED_WORST_RATIO) * (ns + nl) * U * sigma1
    e = (4 * (D + 4) + 2 * (ns + nl) + 13) * U * g
    b = np.sqrt(ns) * np.sqrt(ns * nl) * 2 * e
    out = {"trace_sqrt": (a + b) / np.sqrt((n1 - 1.0) * (n2 - 1.0))}
    dmu = []
    for key, x, n in (("trace1", x1, n1), ("trace2", x2, n2)):
        s = ref[key] * (n - 1)
        dmu.append((n + 1) * U * float(x.max()))
        out[key] = 2 * ((D + n + 3) * U * s + 2 * np.sqrt(n * D * s) * dmu[-1]) / (n - 1)
    d = x1.mean(axis=0) - x2.mean(axis=0)
    dd = 2 * (dmu[0] + dmu[1]) + U * float(np.abs(d).max())
    out["mean_term"] = 2 * np.sqrt(D * ref["mean_term"]) * dd + 2 * (D + 2) * U * ref["mean_term"]
    out["fid"] = (out["mean_term"] + out["trace1"] + out["trace2"] + 2 * out["trace_sqrt"]
                  + 3 * U * (ref["mean_term"] + ref["trace1"] + ref["trace2"] + 2 * ref["trace_sqrt"]))
    return {k: float(v) for k, v in out.items()}


# ---- the GPU case list of the Jacobi stage (tests/test_gpu_frechet.py; tests/test_frechet_cpu.py records the restatement's error on it) ------
def hadamard(k):
    h = np.ones((1, 1))
    for _ in range(k):
        h = np.block([[h, h], [h, -h]])
    return h


def jacobi_cases():
    """name -> fp64 matrix (rows are the vectors)."""
    rng = np.random.RandomState(20)
    cases = {
        "1x5": rng.randn(1, 5),
        "2x2": rng.randn(2, 2),
        "63x70": rng.randn(63, 70),
        "64x64": rng.randn(64, 64),
        "130x70": rng.randn(130, 70),
        "4x2049": rng.randn(4, 2049),
        "4x2048": rng.randn(4, 2048),
        "zero_5x9": np.zeros((5, 9)),
        "rank1_9x12": np.outer(rng.randn(9), rng.randn(12)),
    }
    twin = rng.randn(6, 10)
    twin[4] = twin[1]
    cases["twin_rows_6x10"] = twin
    cases["hadamard_16x16"] = np.arange(1, 17, dtype=np.float64)[::-1, None] * hadamard(4)
    q1, _ = np.linalg.qr(rng.randn(24, 24))
    q2, _ = np.linalg.qr(rng.randn(24, 24))
    cases["graded_24x24"] = (q1 * np.logspace(0, -12, 24)) @ q2.T
    return cases


HADAMARD_SIGMA = 4.0 * np.arange(1, 17, dtype=np.float64)[::-1]      # |k h| = k sqrt(16)

# the worst max_i |sigma_i - sigma_i^svd| / ((m + n) 2^-53 sigma_1) of THIS restatement over jacobi_cases(), recorded by
# tests/test_frechet_cpu.py::test_restatement_against_lapack (which asserts that it still holds), and the GPU tolerance's K = 8 x that: the
# device adds in another order than LAPACK, not in another order than this file
RECORDED_WORST_RATIO = 0.885         # measured 0.8844 (the 2 x 2 case; 0.73 at 130 x 70, 0.67 on the graded matrix, 0.47 at 64 x 64)
K_GPU = 8 * RECORDED_WORST_RATIO


def sv_tolerance(shape, sigma1, K):
    return K * (shape[0] + shape[1]) * U * sigma1
