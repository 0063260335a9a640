"""Feature rows as a strided view of a NaN-poisoned device buffer (tests/test_gpu_kid.py, tests/test_gpu_prdc.py): one NaN read by a kernel
would show in its result."""
import torch


def padded(a, ld, rows_after, dev="cuda:0"):
    """The rows of `a` as a view of a wider, longer device buffer: padding columns and the rows after n hold NaN."""
    n, d = a.shape
    buf = torch.full((n + rows_after, ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:n, :d] = torch.from_numpy(a).to(dev)
    return buf[:n, :d]
