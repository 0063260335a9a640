"""numpy restatement of wu/swd.py: the sliced Wasserstein distance on Laplacian-pyramid patches.  The oracle of tests/test_swd_cpu.py and
tests/test_gpu_swd.py; it imports nothing from the package but the host-side draws and checks (wu.swd.draw / check_levels / default_levels
are plain numpy and are themselves pinned by the CPU tests).

All pyramid arithmetic is float64 and every operation is rounded on its own: numpy evaluates ``a + f * v`` as a product and a sum, which is
what the kernels do under ``fp contract(off)``."""
import numpy as np

F = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
D = 147


def mirror_index(i, n):
    """i < 0 -> -i, i >= n -> 2 (n - 1) - i (no repeated edge sample)."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def mapped(images, scale, shift):
    """Widen to float64, then v * scale + shift in two roundings.  images: float32 / uint8 array, or bf16 given as float32 values."""
    return np.asarray(images).astype(np.float64) * np.float64(scale) + np.float64(shift)


def _pass(g, taps, axis):
    n = g.shape[axis]
    idx = np.arange(n)
    acc = taps[0] * np.take(g, mirror_index(idx - 2, n), axis=axis)
    for t in range(1, 5):
        acc = acc + taps[t] * np.take(g, mirror_index(idx - 2 + t, n), axis=axis)
    return acc


def separable(g, taps):
    """Along H (axis -2) first, then along W (axis -1), taps in ascending order."""
    return _pass(_pass(g, taps, g.ndim - 2), taps, g.ndim - 1)


def blur(g):
    return separable(g, F)


def down(g):
    return blur(g)[..., ::2, ::2]


def up(g):
    z = np.zeros(g.shape[:-2] + (2 * g.shape[-2], 2 * g.shape[-1]), dtype=np.float64)
    z[..., ::2, ::2] = g
    return separable(z, 2.0 * F)


def laplacian_pyramid(g0, levels):
    """[L_0 .. L_{levels-1}] of the mapped float64 images (N, 3, H, W)."""
    out, g = [], g0
    for l in range(levels):
        if l == levels - 1:
            out.append(g)
        else:
            g1 = down(g)
            out.append(g - up(g1))
            g = g1
    return out


def gather(lap, pos):
    """(N P, 147) float32 descriptors of one level: lap (N, 3, H, W) float64, pos (N, P, 2) centres (cy, cx)."""
    n, p = pos.shape[:2]
    out = np.empty((n, p, 3, 7, 7), dtype=np.float32)
    for i in range(n):
        for k in range(p):
            cy, cx = int(pos[i, k, 0]), int(pos[i, k, 1])
            out[i, k] = lap[i, :, cy - 3:cy + 4, cx - 3:cx + 4].astype(np.float32)
    return out.reshape(n * p, D)


def descriptors(images, positions, scale, shift, levels):
    """List over levels of (N P, 147) float32."""
    lap = laplacian_pyramid(mapped(images, scale, shift), levels)
    return [gather(lap[l], positions[l]) for l in range(levels)]


def statistics(desc):
    """(mu, sigma): per channel over its 49 m float32 values, in float64; population standard deviation."""
    v = desc.astype(np.float64).reshape(-1, 3, 49)
    mu = v.mean(axis=(0, 2))
    sigma = np.sqrt(np.square(v - mu[None, :, None]).mean(axis=(0, 2)))
    return mu, sigma


def normalize(desc, mu=None, sigma=None):
    """float32((double(v) - mu_c) / sigma_c); a channel with sigma_c == 0 becomes 0."""
    if mu is None:
        mu, sigma = statistics(desc)
    v = desc.astype(np.float64).reshape(-1, 3, 49)
    safe = np.where(sigma == 0.0, 1.0, sigma)
    out = ((v - mu[None, :, None]) / safe[None, :, None]).astype(np.float32)
    out[:, sigma == 0.0, :] = 0.0
    return out.reshape(-1, D)


def sorted_projections(desc, dirs):
    """(ndirs, m) float64: row j = sort(desc @ dirs[j]), products and sums in float64 on the float32 operands."""
    return np.sort(dirs.astype(np.float64) @ desc.astype(np.float64).T, axis=1)


def wasserstein_1d(a, b):
    """mean |sort(a) - sort(b)| of two equally long 1-D samples."""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        raise ValueError("unequal sample counts")
    return float(np.mean(np.abs(a - b)))


def sliced_wasserstein(d1, d2, dirs):
    """(ndirs,) float64."""
    if d1.shape != d2.shape:
        raise ValueError("unequal descriptor counts")
    return np.mean(np.abs(sorted_projections(d1, dirs) - sorted_projections(d2, dirs)), axis=1)


def swd_levels(images_a, images_b, positions, dirs, scale, shift, levels):
    """Per-level SWD (not yet times 1e3) of two image sets under given draws."""
    da = descriptors(images_a, positions, scale, shift, levels)
    db = descriptors(images_b, positions, scale, shift, levels)
    return np.array([sliced_wasserstein(normalize(a), normalize(b), dirs).mean() for a, b in zip(da, db)])


# ---- the independent formulation the CPU test compares blur / up against: np.pad(mode='reflect') and an explicit 5 x 5 loop ----
def blur_2d_loop(g, taps=F):
    """g (H, W) float64 -> sum_{s,t} taps[s] taps[t] g[y - 2 + s, x - 2 + t] over the reflect-padded image."""
    h, w = g.shape
    pad = np.pad(g, 2, mode="reflect")
    out = np.zeros((h, w), dtype=np.float64)
    for s in range(5):
        for t in range(5):
            out += (taps[s] * taps[t]) * pad[s:s + h, t:t + w]
    return out


def up_2d_loop(g):
    z = np.zeros((2 * g.shape[0], 2 * g.shape[1]), dtype=np.float64)
    z[::2, ::2] = g
    return blur_2d_loop(z, 2.0 * F)
