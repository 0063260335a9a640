"""Device buffers for the kernel-level GPU tests: outputs inside NaN-filled buffers with guard floats on both sides, inputs that must
come back bit-identical, and the ctypes arrays of the _multi entry points."""
import ctypes

import numpy as np
import torch

GUARD = 32
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


class Guarded:
    """n floats inside a NaN-filled buffer with GUARD floats on both sides (optionally initialised from a host array)."""

    def __init__(self, n, init=None):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), NAN, dtype=torch.float32, device=_dev())
        self.view = self.buf[GUARD:GUARD + self.n]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def numpy(self, what, shape=None):
        """The payload, after asserting that both guards are still NaN."""
        host = self.buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + self.n:]).all(), f"{what}: wrote outside its buffer"
        out = host[GUARD:GUARD + self.n].copy()
        return out.reshape(shape) if shape is not None else out

    def untouched(self, what):
        assert np.isnan(self.buf.cpu().numpy()).all(), f"{what}: written although the call was rejected / the output is off"


class Input:
    """A device copy of a host array that must come back bit-identical."""

    def __init__(self, a):
        self.host = np.ascontiguousarray(a, dtype=np.float32)
        self.dev = torch.from_numpy(self.host).to(_dev())

    @property
    def ptr(self):
        return self.dev.data_ptr()

    def unchanged(self, what):
        assert np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host.view(np.uint32)), f"{what}: input modified"


def _lib():
    from wu import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _P(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _I(vals):
    return (ctypes.c_int * len(vals))(*vals)
