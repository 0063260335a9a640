"""Feature rows on the GPU: what the metrics on InceptionV3 features (wu.fid, wu.kid, wu.prdc) share.

``as_rows`` is the one check of "(n, D) float32 CUDA tensor with unit column stride" (any row stride) that the kernels' wrappers rely on;
``FeatureBank`` keeps such rows on the device, appended batch by batch.  There is no host fallback."""
import numpy as np
import torch


def as_rows(f, who):
    """The (n, D) rows of a FeatureBank or of a tensor; a ValueError naming ``who`` when they are not what the kernels read."""
    f = f.features if isinstance(f, FeatureBank) else f
    if not torch.is_tensor(f) or not f.is_cuda or f.dtype != torch.float32 or f.dim() != 2 or f.stride(1) != 1:
        raise ValueError(f"{who}: expected a FeatureBank or an (n, D) float32 CUDA tensor with unit column stride")
    return f


class FeatureBank:
    """Feature rows kept on the GPU, appended batch by batch.  ``features`` is the (n, D) view of the rows so far, ``n`` their number; the
    device buffer doubles when it is full.  ``save_npz`` / ``load_npz`` use the key ``features`` (float32).  ``resize`` is the rule the
    images reached the network under (``InceptionV3(resize=...)``); anything but ``"legacy"`` is recorded under the key ``resize``, and a
    file without that key is legacy."""

    def __init__(self, dim=None, resize="legacy"):
        self.dim = dim
        self.n = 0
        self._buf = None
        self.resize = resize

    def append(self, feats):
        feats = as_rows(feats, "FeatureBank.append")
        b, d = feats.shape
        if self.dim is None:
            self.dim = d
        elif d != self.dim:
            raise ValueError(f"FeatureBank: feature width {d} differs from the bank's {self.dim}")
        if self._buf is None or self.n + b > self._buf.shape[0]:
            cap = max(64, self.n + b, 2 * (0 if self._buf is None else self._buf.shape[0]))
            buf = torch.empty(cap, d, dtype=torch.float32, device=feats.device)
            if self.n:
                buf[:self.n].copy_(self._buf[:self.n])
            self._buf = buf
        self._buf[self.n:self.n + b].copy_(feats)
        self.n += b

    @property
    def capacity(self):
        return 0 if self._buf is None else self._buf.shape[0]

    @property
    def features(self):
        if self._buf is None:
            raise ValueError("FeatureBank: no rows yet")
        return self._buf[:self.n]

    def save_npz(self, path):
        np.savez(path, features=self.features.cpu().numpy(), **({} if self.resize == "legacy" else {"resize": np.array(self.resize)}))

    @classmethod
    def load_npz(cls, path, device="cuda"):
        with np.load(path) as f:
            if "features" not in f:
                raise ValueError(f"{path}: no 'features' array (keys {sorted(f.keys())}); KID needs the feature rows, not mu / sigma")
            a = np.ascontiguousarray(f["features"], dtype=np.float32)
            rule = str(f["resize"]) if "resize" in f else "legacy"
        if a.ndim != 2:
            raise ValueError(f"{path}: 'features' has shape {a.shape}, expected (n, D)")
        bank = cls(a.shape[1], rule)
        if a.shape[0]:
            bank.append(torch.from_numpy(a).to(device))
        return bank
