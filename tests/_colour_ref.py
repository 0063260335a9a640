"""numpy restatement of wu.colour (csrc/colour_ot.hip): histogram matching and sliced optimal transport of pixel colours.  Every operation
is a float64 numpy ufunc of its own, in the order the module docstring fixes, so the kernels -- which do the same operations without FMA --
must reproduce these numbers bit for bit.  The rotations are an input: LAPACK's bits never enter a comparison."""
import numpy as np


def load_state(x, scale, shift, L):
    """(B, 3, H, W) values as the kernel sees them -> (B, 3, n) float64 in [0, 1] units."""
    x = np.asarray(x)
    s = (x.astype(np.float64) * scale + shift) / L
    return s.reshape(x.shape[0], 3, -1)


def project(R, s):
    """s (3, m) -> keys (3, m): key_a = (R[a][0] s_0 + R[a][1] s_1) + R[a][2] s_2."""
    return np.stack([(R[a, 0] * s[0] + R[a, 1] * s[1]) + R[a, 2] * s[2] for a in range(3)])


def ranks(keys, P):
    """Per key of one axis of one image: t = ((lo + hi) P) // (2 n) with lo = #{key' < key}, hi = #{key' <= key}."""
    n = keys.shape[0]
    srt = np.sort(keys)
    lo = np.searchsorted(srt, keys, side="left").astype(np.int64)
    hi = np.searchsorted(srt, keys, side="right").astype(np.int64)
    return ((lo + hi) * np.int64(P)) // np.int64(2 * n)


def step(s, palette, R, step_size=1.0):
    """One iteration on one image: s (3, n), palette (P, 3), R (3, 3) -> the new (3, n)."""
    P = palette.shape[0]
    keys = project(R, s)
    q = np.sort(project(R, np.ascontiguousarray(palette.T)), axis=1)
    delta = np.stack([q[a][ranks(keys[a], P)] - keys[a] for a in range(3)])
    return np.stack([s[c] + step_size * ((delta[0] * R[0, c] + delta[1] * R[1, c]) + delta[2] * R[2, c]) for c in range(3)])


def iterate(s, palette, rotations, step_size=1.0):
    for R in rotations:
        s = step(s, palette, R, step_size)
    return s


def to_bf16(f32):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32; finite values."""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def store(s, value_range, dtype):
    """The state -> output values: dtype "float32", "bfloat16" (as float32 values) or "uint8"."""
    u = np.minimum(np.maximum(s, 0.0), 1.0)
    if isinstance(value_range, str):
        v = np.rint(u * 255.0)
    else:
        lo, hi = float(value_range[0]), float(value_range[1])
        v = lo + u * (hi - lo)
    if dtype == "uint8":
        return np.minimum(np.maximum(np.rint(v), 0.0), 255.0).astype(np.uint8)
    v = v.astype(np.float32)
    return to_bf16(v) if dtype == "bfloat16" else v


def transfer(x, palettes, targets, rotations, step_size, value_range, mapping, dtype):
    """x (B, 3, H, W) as the kernel sees it, palettes (C, P, 3), targets (R,), rotations (K, 3, 3), mapping = (scale, shift, L)
    -> (R, B, 3, H, W)."""
    b, _, h, w = x.shape
    s0 = load_state(x, *mapping)
    out = [[store(iterate(s0[i], palettes[t], rotations, step_size), value_range, dtype).reshape(3, h, w) for i in range(b)] for t in targets]
    return np.array(out)
