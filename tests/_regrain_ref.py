"""numpy restatement of the regraining pass and the linear colour maps of wu.colour (csrc/colour_regrain.hip).  Every operation is a float64
numpy ufunc of its own, in the order include/wu_kernels.h fixes, so the kernels -- which do the same operations without FMA -- must reproduce
these numbers bit for bit.  Nothing here knows of tiles, halos or workgroups."""
import numpy as np

import _colour_ref as CR

DEFAULT_ITERS = (4, 16, 32, 64, 64, 64)
EPS52 = 2.0 ** -52
NBRS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # up, down, left, right


# ----------------------------------------------------------------------------------------------
# regraining
# ----------------------------------------------------------------------------------------------
def level_sizes(h, w, n_iters, min_side):
    """[(h_0, w_0), ..]: level l + 1 exists iff l + 1 < n_iters and both ceil(h_l / 2) and ceil(w_l / 2) exceed min_side."""
    out = [(h, w)]
    while len(out) < n_iters and -(-h // 2) > min_side and -(-w // 2) > min_side:
        h, w = -(-h // 2), -(-w // 2)
        out.append((h, w))
    return out


def sh(a, dy, dx):
    """a (.., h, w) read at (y + dy, x + dx), clamped at the image edge."""
    h, w = a.shape[-2:]
    y = np.clip(np.arange(h) + dy, 0, h - 1)
    x = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[..., y[:, None], x[None, :]]


def _down_axis(a, axis):
    n = a.shape[axis]
    d = np.arange(-(-n // 2))
    return (np.take(a, 2 * d, axis) + np.take(a, np.minimum(2 * d + 1, n - 1), axis)) * 0.5


def down(a):
    """(.., h, w) -> (.., ceil(h / 2), ceil(w / 2)): rows first (pairs of rows are averaged), then columns."""
    return _down_axis(_down_axis(a, -2), -1)


def _up_axis(a, n, axis):
    nc = a.shape[axis]
    d = np.arange(n)
    o = np.clip(np.where(d % 2 == 0, d // 2 - 1, d // 2 + 1), 0, nc - 1)
    return np.take(a, d // 2, axis) * 0.75 + np.take(a, o, axis) * 0.25


def up(a, h, w):
    """(.., hc, wc) -> (.., h, w): rows first, then columns."""
    return _up_axis(_up_axis(a, h, -2), w, -1)


def weights(I0, IT, level, smoothness):
    """(psi-free) pieces of one level: phi_j (4, h, w), den (h, w), b (3, h, w) from I0, IT (3, h, w)."""
    gx = sh(I0, 0, 1) - sh(I0, 0, -1)
    gy = sh(I0, 1, 0) - sh(I0, -1, 0)
    q = gx * gx + gy * gy
    dI = np.sqrt((q[0] + q[1]) + q[2])
    psi = np.minimum((256.0 * dI) / 5.0, 1.0)
    phi = (30.0 * 2.0 ** -level) / (1.0 + (10.0 * dI) / smoothness)
    pj = [(sh(phi, dy, dx) + phi) * 0.5 for dy, dx in NBRS]
    den = ((((psi + pj[0]) + pj[1]) + pj[2]) + pj[3]) + EPS52
    b = psi * IT
    for j, (dy, dx) in enumerate(NBRS):
        b = b + pj[j] * (I0 - sh(I0, dy, dx))
    return pj, den, b


def solve(IR, I0, IT, iters, level, smoothness):
    pj, den, b = weights(I0, IT, level, smoothness)
    for _ in range(iters):
        a = b
        for j, (dy, dx) in enumerate(NBRS):
            a = a + pj[j] * sh(IR, dy, dx)
        IR = (a / den) * 0.8 + 0.2 * IR
    return IR


def _rec(IR, I0, IT, level, sizes, iters, smoothness, replace):
    if level + 1 < len(sizes):
        c0 = down(IR)
        c1 = _rec(c0, down(I0), down(IT), level + 1, sizes, iters, smoothness, replace)
        h, w = IR.shape[-2:]
        IR = up(c1, h, w) if replace else IR + up(c1 - c0, h, w)
    return solve(IR, I0, IT, iters[level], level, smoothness)


def regrain(I0, IT, iters=DEFAULT_ITERS, smoothness=1.0, min_side=20, replace=False):
    """I0, IT (3, h, w) float64 in [0, 1] units -> IR (3, h, w), not clipped.  ``replace=True`` is the recursion of the published code (the
    coarse solution replaces IR), kept to show why the kernels do not use it."""
    I0, IT = np.asarray(I0, dtype=np.float64), np.asarray(IT, dtype=np.float64)
    sizes = level_sizes(I0.shape[1], I0.shape[2], len(iters), min_side)
    return _rec(IT, I0, IT, 0, sizes, iters, float(smoothness), replace)


# ----------------------------------------------------------------------------------------------
# moments and linear maps
# ----------------------------------------------------------------------------------------------
def _lanes(v):
    """(.., m 256) -> (..): lane t adds v[t], v[t + 256], .. in order to +0.0; the lanes fold by v[t] += v[t + s], s = 128 .. 1."""
    v = v.reshape(v.shape[:-1] + (-1, 256))
    acc = np.zeros(v.shape[:-2] + (256,))
    for j in range(v.shape[-2]):
        acc = acc + v[..., j, :]
    s = 128
    while s >= 1:
        acc = acc[..., :s] + acc[..., s:2 * s]
        s //= 2
    return acc[..., 0]


def _pad(v, m):
    n = v.shape[-1]
    return np.concatenate([v, np.zeros(v.shape[:-1] + (-n % m,))], axis=-1)


def fixed_sum(v):
    """The sum over the last axis in the order the kernels use, which depends on its length alone."""
    v = _pad(np.asarray(v, dtype=np.float64), 4096)
    chunks = _lanes(v.reshape(v.shape[:-1] + (-1, 4096)))
    return _lanes(_pad(chunks, 256))


def moments(s):
    """s (3, n) -> mu (3,), Sigma (3, 3): two passes, the population form."""
    n = float(s.shape[1])
    mu = fixed_sum(s) / n
    d = s - mu[:, None]
    cov = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            cov[a, b] = cov[b, a] = fixed_sum(d[a] * d[b]) / n
    return mu, cov


def jacobi(M):
    """Cyclic Jacobi on the upper triangle of a 3 x 3 symmetric matrix: exactly 8 sweeps over (0,1), (0,2), (1,2).  -> (lam (3,), V (3, 3))."""
    a = np.array([[M[min(i, j), max(i, j)] for j in range(3)] for i in range(3)], dtype=np.float64)
    v = np.eye(3)
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(over="ignore"):
        for _ in range(8):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (two * apq)
                t = (one if theta >= 0.0 else -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                a[p, p] = a[p, p] - t * apq
                a[q, q] = a[q, q] + t * apq
                a[p, q] = a[q, p] = 0.0
                arp, arq = a[r, p], a[r, q]
                a[r, p] = a[p, r] = c * arp - s * arq
                a[r, q] = a[q, r] = s * arp + c * arq
                for i in range(3):
                    vip, viq = v[i, p], v[i, q]
                    v[i, p] = c * vip - s * viq
                    v[i, q] = s * vip + c * viq
    return np.array([a[0, 0], a[1, 1], a[2, 2]]), v


def fsym(V, f):
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            out[i, j] = out[j, i] = ((V[i, 0] * f[0]) * V[j, 0] + (V[i, 1] * f[1]) * V[j, 1]) + (V[i, 2] * f[2]) * V[j, 2]
    return out


def matmul(X, Y):
    return np.array([[(X[i, 0] * Y[0, j] + X[i, 1] * Y[1, j]) + X[i, 2] * Y[2, j] for j in range(3)] for i in range(3)])


def linear_map(cov_s, cov_t, method, eps_var=1e-10):
    """The 3 x 3 matrix A of ``s <- mu_t + A (s - mu_s)``."""
    if method == "meanstd":
        return np.diag([np.sqrt(cov_t[c, c] / max(cov_s[c, c], eps_var)) for c in range(3)])
    assert method == "mkl"
    lam, V = jacobi(cov_s)
    f = np.sqrt(np.maximum(lam, eps_var))
    S, Si = fsym(V, f), fsym(V, 1.0 / f)
    M = matmul(matmul(S, cov_t), S)
    lam, U = jacobi(M)
    Mr = fsym(U, np.sqrt(np.maximum(lam, 0.0)))
    return matmul(matmul(Si, Mr), Si)


def linear_apply(s, mom_s, mom_t, method, eps_var=1e-10):
    """s (3, n) -> the mapped (3, n)."""
    A = linear_map(mom_s[1], mom_t[1], method, eps_var)
    d = s - mom_s[0][:, None]
    return np.stack([((A[c, 0] * d[0] + A[c, 1] * d[1]) + A[c, 2] * d[2]) + mom_t[0][c] for c in range(3)])


# ----------------------------------------------------------------------------------------------
# the whole of wu.colour.transfer / wu.colour.regrain
# ----------------------------------------------------------------------------------------------
def transfer(x, palettes, targets, rotations, step_size, value_range, mapping, dtype, method="idt", regrain_args=None, eps_var=1e-10):
    """As _colour_ref.transfer, with ``method`` and an optional regraining pass (a dict of regrain()'s keywords, or None)."""
    b, _, h, w = x.shape
    s0 = CR.load_state(x, *mapping)
    pal_mom = [moments(np.ascontiguousarray(p.T)) for p in palettes] if method != "idt" else None
    out = []
    for t in targets:
        row = []
        for i in range(b):
            if method == "idt":
                s = CR.iterate(s0[i], palettes[t], rotations, step_size)
            else:
                s = linear_apply(s0[i], moments(s0[i]), pal_mom[t], method, eps_var)
            if regrain_args is not None:
                s = regrain(s0[i].reshape(3, h, w), s.reshape(3, h, w), **regrain_args).reshape(3, -1)
            row.append(CR.store(s, value_range, dtype).reshape(3, h, w))
        out.append(row)
    return np.array(out)


def regrain_images(original, transferred, value_range, mapping, dtype, **kw):
    """original (B, 3, H, W), transferred (B, 3, H, W) or (R, B, 3, H, W), as the kernels see them -> the shape of ``transferred``."""
    b, _, h, w = original.shape
    s0 = CR.load_state(original, *mapping)
    y = transferred.reshape((-1,) + transferred.shape[-4:])
    out = np.array([[CR.store(regrain(s0[i].reshape(3, h, w), CR.load_state(yr[i:i + 1], *mapping)[0].reshape(3, h, w), **kw).reshape(3, -1),
                              value_range, dtype).reshape(3, h, w) for i in range(b)] for yr in y])
    return out.reshape(transferred.shape)
