"""Inputs shared by tests/test_colour_cpu.py and tests/test_gpu_colour.py: images, palettes and tie cases, all drawn from fixed seeds."""
import numpy as np

RANK_NP = [(1, 1), (1, 7), (7, 1), (5, 16), (16, 5)]          # (n, P) at which t must stay in 0..P-1


def images(b, h, w, seed):
    """(b, 3, h, w) float32 in [-1, 1]: a colour cast per image under noise, so that images and channels differ."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.5, 0.5, (b, 3, 1, 1)) + rng.uniform(-0.5, 0.5, (b, 3, h, w))
    return x.astype(np.float32)


def images_u8(b, h, w, seed):
    return np.round((images(b, h, w, seed) + 1) * 127.5).astype(np.uint8)


def noise_u8(b, h, w, seed, levels=7):
    """uint8 noise over a handful of levels: heavy ties on every axis."""
    return (np.random.RandomState(seed).randint(0, levels, (b, 3, h, w)) * (255 // (levels - 1))).astype(np.uint8)


def flat(b, h, w, colour=(0.25, -0.5, 0.75)):
    return np.broadcast_to(np.asarray(colour, dtype=np.float32).reshape(1, 3, 1, 1), (b, 3, h, w)).copy()


def two_colour(b, h, w, seed):
    """Two colours in unequal shares, scattered."""
    rng = np.random.RandomState(seed)
    mask = rng.uniform(size=(b, 1, h, w)) < 0.3
    a = np.asarray([0.8, -0.2, 0.1], dtype=np.float32).reshape(1, 3, 1, 1)
    c = np.asarray([-0.6, 0.4, 0.9], dtype=np.float32).reshape(1, 3, 1, 1)
    return np.where(mask, a, c).astype(np.float32)


def palettes(c, p, seed):
    """(c, p, 3) float64 in [0, 1]: a Gaussian blob per class, clipped; classes differ in mean and spread."""
    rng = np.random.RandomState(seed)
    mean = rng.uniform(0.2, 0.8, (c, 1, 3))
    spread = rng.uniform(0.05, 0.3, (c, 1, 3))
    return np.clip(mean + spread * rng.randn(c, p, 3), 0.0, 1.0)


def repeated_palette(c, p, colour=(0.5, 0.125, 0.875)):
    return np.broadcast_to(np.asarray(colour, dtype=np.float64).reshape(1, 1, 3), (c, p, 3)).copy()


def distinct_integer_image(n, seed):
    """(1, 3, 1, n) float32 whose every channel is a permutation of 0..n-1 scaled into [0, 1] exactly (n a power of two)."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.permutation(n) for _ in range(3)]).reshape(1, 3, 1, n).astype(np.float32) / np.float32(n)
