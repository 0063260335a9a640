"""Radial (azimuthally averaged) power spectrum of real against generated images: where in frequency do the outputs depart from the
photographs?  (Durall et al., CVPR 2020, "Watch your up-convolution"; Dzanic et al., NeurIPS 2020; Zhang et al., WIFS 2019 for the mean 2-D
spectrum picture.)  Up-sampling residue, dropout grain, colour-transfer banding and the JPEG grid each leave a mark here that FID or SSIM
only register as a small shift.

    y = luma(images)                                    # (N, H, W) float64 CUDA
    p = profiles(images)                                # (N, K) float64 CUDA: mean power per radial bin
    idx, count, freq = radial_bins(H, W)
    r = compare(SpectrumBank().add(real), SpectrumBank().add(fake))      # SpectrumResult
    python -m wu.spectrum DIR_A DIR_B [--size S] [--filter F] [--window hann] [--gpu-decode] [--json out.json] [--mean-spectrum out.png]

Semantics, in full (tests/_spectrum_ref.py restates them in numpy).  fp64 throughout, every operation outside the two matrix products rounded
on its own.

Input.  (N, C, H, W), C 1 or 3, 1 <= H, W <= 1024, float32, bfloat16 or uint8, any strides.  ``s = (double(v) * scale + shift) / L`` with
``wu.paired.range_mapping(value_range)``.  Luma: ``y = (0.299 s_R + 0.587 s_G) + 0.114 s_B``; C = 1: ``y = s``.

Window.  ``"none"`` (the default, Durall's choice) or ``"hann"``: ``y[i][j] = (y[i][j] * wh[i]) * ww[j]`` with ``w_n[k] = 0.5 - 0.5 c_n[k]``.

Twiddle tables (``twiddles(n)``, built on the host, uploaded as data).  ``c_n[k], s_n[k]`` = cos, sin of 2 pi k / n: write ``8 k = q n + r``
in integers; take ``math.cos / math.sin`` of ``(r / n) pi / 4`` when q is even, and of ``((n - r) / n) pi / 4`` with the roles of cos and sin
swapped when q is odd; rotate by ``q // 2`` quarter turns, ``(c, s) -> (-s, c)``.  Multiples of a quarter turn are exactly 0 and +-1.

Half spectrum.  ``Wh = W // 2 + 1``; ``Tr[i][v] = sum_j y[i][j] c_W[(v j) mod W]``, ``Ti[i][v] = -sum_j y[i][j] s_W[(v j) mod W]``;
``Xr[u][v] = sum_i (c_H[(u i) mod H] Tr[i][v] + s_H[(u i) mod H] Ti[i][v])``, ``Xi[u][v] = sum_i (c_H[(u i) mod H] Ti[i][v] -
s_H[(u i) mod H] Tr[i][v])``; ``P = Xr Xr + Xi Xi``.  Mirror weight: 2 for 0 < v < W / 2, 1 for v = 0 and (W even) v = W / 2.

Radial bin, integers only.  ``fu = u if u <= H // 2 else u - H``, ``fv = v``, ``M = min(H, W)``, ``q = fu^2 W^2 + fv^2 H^2``,
``k = isqrt(q M^2) // (H W)``; for H = W this is ``isqrt(fu^2 + fv^2)``.  ``K = largest k + 1``: the corner bins beyond Nyquist are kept.
``count[k]`` is the sum of the mirror weights in the bin (the counts sum to H W), ``freq[k] = k / M`` cycles per pixel.

Profile.  ``prof[n][k] = (sum over the bin of weight P) / count[k] / (H W)^2``.  The mean 2-D spectrum of a set is
``(sum_n P[n]) / N / (H W)^2``, (H, Wh), summed over n ascending.

Comparison (``SpectrumBank``, ``compare``).  ``dB = 10 log10(prof)``.  A bank keeps, per bin, ``sum_n dB`` and ``sum_n dB^2`` over the images
that have no bin of zero power in 1 .. M // 2; the others are counted in ``flat`` and left out.  Over bins 1 .. M // 2: the mean and the
population standard deviation (``sqrt(max(sum dB^2 / n - mean^2, 0))``) of each side, ``d = mean_db_b - mean_db_a``, ``lsd = sqrt(mean d^2)``,
``bands`` = the mean of d over the lower, middle and upper third of those bins (``[0, nb // 3)``, ``[nb // 3, 2 nb // 3)``, the rest; a
negative upper band means blurrier than side a, a positive one grain or artefacts), ``peak = (max |d|, its frequency)``: a periodic artefact
shows there.

Kernels (csrc/spectrum.hip): two GEMM stages on the fp64 matrix cores with the twiddle operands generated from the 1-D tables in LDS, luma and
window applied while the row stage stages its tile (no fp64 plane in memory), the radial sums per tile in a fixed order and folded over tiles
ascending: no atomics, two runs give the same bits, and ``max_images`` (how many images share a workspace) changes the memory in use and
nothing else.  CUDA tensors only for anything that touches pixels: there is no CPU fallback."""
import collections
import math

import numpy as np
import torch

from . import _lib
from .layout import stream_ptr
from .paired import U8, range_mapping

MAX_SIDE = 1024
MAX_IMAGES = 65535                      # images per library call
WORKSPACE_BYTES = 256 << 20             # the default max_images keeps the workspace within this
WINDOWS = ("none", "hann")
_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: U8}

SpectrumResult = collections.namedtuple("SpectrumResult", "freq mean_db_a mean_db_b std_db_a std_db_b lsd bands peak count_a count_b "
                                        "flat_a flat_b")


def twiddles(n):
    """(c, s): float64 numpy tables of cos and sin of 2 pi k / n, k < n, by the rule of the module docstring."""
    n = int(n)
    c, s = np.empty(n), np.empty(n)
    for k in range(n):
        q, r = divmod(8 * k, n)
        if q % 2 == 0:
            a = (r / n) * (math.pi / 4)
            ck, sk = math.cos(a), math.sin(a)
        else:
            a = ((n - r) / n) * (math.pi / 4)
            ck, sk = math.sin(a), math.cos(a)
        for _ in range(q // 2):
            ck, sk = -sk, ck
        c[k], s[k] = ck, sk
    return c + 0.0, s + 0.0             # no negative zeros


def window_table(n):
    """The Hann table of n doubles: 0.5 - 0.5 c_n[k]."""
    return 0.5 - 0.5 * twiddles(n)[0]


def _check_side(h, w, what):
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"{what}: image sides must be in 1..{MAX_SIDE}, got {h} x {w}")


def radial_bins(H, W):
    """(bin index (H, Wh) int32, count (K,) int64, freq (K,) float64 = k / min(H, W) cycles per pixel), numpy, integers only."""
    H, W = int(H), int(W)
    _check_side(H, W, "radial_bins")
    M = min(H, W)
    u = np.arange(H, dtype=np.int64)
    fu = np.where(u <= H // 2, u, u - H)[:, None]
    fv = np.arange(W // 2 + 1, dtype=np.int64)[None, :]
    x = (fu * fu * W * W + fv * fv * H * H) * (M * M)          # below 2^59
    r = np.sqrt(x.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > x, r - 1, r)                          # the float root is off by at most one either way
    r = np.where((r + 1) * (r + 1) <= x, r + 1, r)
    assert bool(np.all((r * r <= x) & ((r + 1) * (r + 1) > x)))
    idx = (r // (H * W)).astype(np.int32)
    weight = np.where((fv > 0) & (2 * fv < W), 2, 1).astype(np.int64)
    count = np.zeros(int(idx.max()) + 1, dtype=np.int64)
    np.add.at(count, idx, np.broadcast_to(weight, idx.shape))
    return idx, count, np.arange(count.shape[0]) / M


def _require_cuda(*tensors):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError("wu.spectrum: CUDA tensors only -- no CPU fallback")


_TABLES = {}


def _tables(n, device):
    """(c_n, s_n, hann_n) on the device, cached per (n, device)."""
    key = (int(n), str(device))
    if key not in _TABLES:
        c, s = twiddles(n)
        _TABLES[key] = tuple(torch.from_numpy(t).to(device) for t in (c, s, 0.5 - 0.5 * c))
    return _TABLES[key]


def _check_images(images, window, what):
    _require_cuda(images)
    if images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError(f"{what}: images must be (N, C, H, W) with C 1 or 3, got {tuple(images.shape)}")
    if images.dtype not in _DTYPES:
        raise ValueError(f"{what}: float32, bfloat16 or uint8, got {images.dtype}")
    if window not in WINDOWS:
        raise ValueError(f"{what}: window must be one of {WINDOWS}, got {window!r}")
    n, c, h, w = images.shape
    _check_side(h, w, what)
    if n < 1:
        raise ValueError(f"{what}: no images")
    return n, c, h, w


def _window_ptrs(window, h, w, dev):
    if window == "none":
        return None, None, ()
    wh, ww = _tables(h, dev)[2], _tables(w, dev)[2]
    return wh.data_ptr(), ww.data_ptr(), (wh, ww)


def luma(images, value_range=(-1, 1), window="none"):
    """(N, H, W) float64 CUDA: the mapped, windowed luma plane of every image (the first step of the two-step path; ``profiles`` never
    writes it)."""
    n, c, h, w = _check_images(images, window, "luma")
    scale, shift, L = range_mapping(value_range)
    images = images.detach()
    dev = images.device
    out = torch.empty(n, h, w, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ph, pw, _keep = _window_ptrs(window, h, w, dev)
        _lib.call("wu_spectrum_luma", images.data_ptr(), *images.stride(), _DTYPES[images.dtype], n, c, h, w, scale, shift, L, ph, pw,
                  out.data_ptr(), stream_ptr())
    return out


def default_max_images(H, W):
    """The largest number of images whose workspace stays within WORKSPACE_BYTES (at least 1)."""
    lib = _lib.load()
    one, two = lib.wu_spectrum_workspace_bytes(1, H, W), lib.wu_spectrum_workspace_bytes(2, H, W)
    k = max(1, 1 + (WORKSPACE_BYTES - one) // max(1, two - one))
    while k > 1 and lib.wu_spectrum_workspace_bytes(int(k), H, W) > WORKSPACE_BYTES:
        k -= 1
    return int(min(k, MAX_IMAGES))


def _run(images, planes, value_range, window, max_images, mean_spectrum):
    """The chunk loop behind ``profiles`` and ``profiles_planes``."""
    if planes:
        _require_cuda(images)
        if images.dim() != 3 or images.dtype != torch.float64:
            raise ValueError(f"profiles_planes: (N, H, W) float64 planes, got {tuple(images.shape)} {images.dtype}")
        images = images.detach().contiguous()
        n, h, w = images.shape
        c = 1
        _check_side(h, w, "profiles_planes")
        if n < 1:
            raise ValueError("profiles_planes: no planes")
    else:
        n, c, h, w = _check_images(images, window, "profiles")
        images = images.detach()
        scale, shift, L = range_mapping(value_range)
    dev = images.device
    lib = _lib.load()
    K = lib.wu_spectrum_bins(h, w)
    chunk = default_max_images(h, w) if max_images is None else int(max_images)
    if chunk < 1:
        raise ValueError(f"profiles: max_images {max_images} must be at least 1")
    chunk = min(chunk, n, MAX_IMAGES)
    if mean_spectrum is not None:
        _require_cuda(mean_spectrum)
        if tuple(mean_spectrum.shape) != (h, w // 2 + 1) or mean_spectrum.dtype != torch.float64 or not mean_spectrum.is_contiguous():
            raise ValueError(f"profiles: mean_spectrum must be a contiguous ({h}, {w // 2 + 1}) float64 tensor (the running sum of P), got "
                             f"{tuple(mean_spectrum.shape)} {mean_spectrum.dtype}")
    ws = torch.empty(lib.wu_spectrum_workspace_bytes(chunk, h, w), dtype=torch.uint8, device=dev)
    out = torch.empty(n, K, dtype=torch.float64, device=dev)
    cw, sw, _ = _tables(w, dev)
    ch, sh, _ = _tables(h, dev)
    sum_ptr = mean_spectrum.data_ptr() if mean_spectrum is not None else None
    with torch.cuda.device(dev):
        ph, pw, _keep = _window_ptrs(window, h, w, dev)
        for n0 in range(0, n, chunk):
            part = images[n0:n0 + chunk]
            if planes:
                _lib.call("wu_spectrum_profiles_planes", part.data_ptr(), part.shape[0], h, w, cw.data_ptr(), sw.data_ptr(), ch.data_ptr(),
                          sh.data_ptr(), K, ws.data_ptr(), out[n0:].data_ptr(), sum_ptr, stream_ptr())
            else:
                _lib.call("wu_spectrum_profiles", part.data_ptr(), *part.stride(), _DTYPES[part.dtype], part.shape[0], c, h, w, scale, shift,
                          L, ph, pw, cw.data_ptr(), sw.data_ptr(), ch.data_ptr(), sh.data_ptr(), K, ws.data_ptr(), out[n0:].data_ptr(),
                          sum_ptr, stream_ptr())
    return out


def profiles(images, value_range=(-1, 1), window="none", max_images=None, mean_spectrum=None):
    """(N, K) float64 CUDA: the radial power profile of every image.  images (N, C, H, W), C 1 or 3, float32, bfloat16 or uint8 CUDA of any
    strides.  ``max_images`` images share one workspace (default: as many as fit ``WORKSPACE_BYTES``); it changes no bit of the result.
    ``mean_spectrum``: a contiguous (H, Wh) float64 CUDA tensor to which ``P[n]`` of every image is ADDED, n ascending (zero it first; divide
    by the count and by ``(H W)^2`` for the mean 2-D spectrum); only then does a 2-D spectrum reach memory."""
    return _run(images, False, value_range, window, max_images, mean_spectrum)


def profiles_planes(planes, max_images=None, mean_spectrum=None):
    """``profiles`` of (N, H, W) float64 CUDA planes as ``luma`` returns them: the second step of the two-step path, the same bits."""
    return _run(planes, True, None, "none", max_images, mean_spectrum)


# ----------------------------------------------------------------------------------------------
# banks and their comparison
# ----------------------------------------------------------------------------------------------
class SpectrumBank:
    """Per radial bin, ``sum_n dB`` and ``sum_n dB^2`` (``dB = 10 log10(prof)``) of a stream of image batches, fp64 on the device: one side
    of ``compare``, or the ``reference=`` of ``wu.evaluate.SpectralDiscrepancy``.  ``add(images)``: (B, C, H, W) CUDA, one image size for
    the whole stream.  ``count`` images were kept; ``flat`` more had a bin of zero power in 1 .. M // 2 and were left out of the sums (read
    either and the device is synchronised).  ``keep_mean_spectrum``: also keep the running sum of the 2-D spectra of ALL images
    (``mean_spectrum()``)."""

    def __init__(self, value_range=(-1, 1), window="none", keep_mean_spectrum=False, max_images=None):
        if window not in WINDOWS:
            raise ValueError(f"SpectrumBank: window must be one of {WINDOWS}, got {window!r}")
        self.value_range, self.window, self.keep_mean_spectrum, self.max_images = value_range, window, bool(keep_mean_spectrum), max_images
        self.shape, self.mapping, self.images = None, None, 0
        self.sum_db = self.sum_db2 = self.kept = self.spectrum_sum = None

    def _open(self, h, w, what):
        mapping = tuple(range_mapping(self.value_range))
        if self.shape is None:
            self.shape, self.mapping = (int(h), int(w)), mapping
        elif self.shape != (h, w) or self.mapping != mapping:
            raise ValueError(f"{what}: {h} x {w} mapped {mapping} after {self.shape[0]} x {self.shape[1]} mapped {self.mapping}")

    @torch.no_grad()
    def add(self, images):
        _require_cuda(images)
        if images.dim() != 4:
            raise ValueError(f"SpectrumBank.add: images must be (B, C, H, W), got {tuple(images.shape)}")
        h, w = images.shape[2:]
        _check_images(images, self.window, "SpectrumBank.add")
        self._open(h, w, "SpectrumBank.add")
        if self.keep_mean_spectrum and self.spectrum_sum is None:
            self.spectrum_sum = torch.zeros(h, w // 2 + 1, dtype=torch.float64, device=images.device)
        prof = profiles(images, self.value_range, self.window, self.max_images, self.spectrum_sum)
        return self._add(prof)

    @torch.no_grad()
    def add_profiles(self, prof, shape):
        """Profiles (B, K) float64 of images of ``shape = (H, W)`` computed elsewhere (any device): the same bookkeeping as ``add``."""
        h, w = (int(v) for v in shape)
        _check_side(h, w, "SpectrumBank.add_profiles")
        K = radial_bins(h, w)[1].shape[0]
        if not torch.is_tensor(prof) or prof.dim() != 2 or prof.shape[1] != K or prof.dtype != torch.float64:
            raise ValueError(f"SpectrumBank.add_profiles: (B, {K}) float64 profiles for {h} x {w}, got "
                             f"{tuple(prof.shape) if torch.is_tensor(prof) else type(prof)}")
        self._open(h, w, "SpectrumBank.add_profiles")
        return self._add(prof)

    def _add(self, prof):
        m = min(self.shape)
        band = prof[:, 1:m // 2 + 1]
        flat = (band == 0).any(1)
        keep = (~flat).to(torch.float64)[:, None]
        db = 10.0 * torch.log10(prof)
        db = torch.where(keep > 0, db, torch.zeros_like(db))     # a flat image adds +0 everywhere, whatever its logs are
        s1, s2 = db.sum(0), (db * db).sum(0)
        if self.sum_db is None:
            self.sum_db, self.sum_db2, self.kept = s1, s2, keep.sum()
        else:
            self.sum_db, self.sum_db2, self.kept = self.sum_db + s1, self.sum_db2 + s2, self.kept + keep.sum()
        self.images += prof.shape[0]
        return self

    @property
    def count(self):
        """Images kept in the sums (``images`` were added)."""
        return 0 if self.kept is None else int(self.kept.item())

    @property
    def flat(self):
        return self.images - self.count

    def signature(self):
        """What two banks must share to be compared: image size, window, value-range mapping."""
        if self.sum_db is None:
            raise RuntimeError("SpectrumBank: no batch has been added yet")
        return {"image size": self.shape, "window": self.window, "value-range mapping": self.mapping}

    def mean_spectrum(self):
        """(H, Wh) float64: ``(sum_n P[n]) / images / (H W)^2`` over all images added."""
        if self.spectrum_sum is None:
            raise RuntimeError("SpectrumBank: built without keep_mean_spectrum, or nothing added yet")
        hw = float(self.shape[0] * self.shape[1])
        return self.spectrum_sum / float(self.images) / (hw * hw)

    @classmethod
    def from_dir(cls, dir, size=None, filter=None, gpu_decode=False, device="cuda:0", batch_size=64, **kwargs):
        """The bank of every .jpg / .png file of ``dir`` in sorted order, read through ``wu.files.read_images`` (``size``, ``filter``,
        ``gpu_decode`` as there); ``kwargs`` go to the constructor.  The value range is the reader's."""
        from .files import image_files, read_images
        files = image_files(dir)
        if not files:
            raise RuntimeError(f"no .jpg / .png images in {dir}")
        bank = cls(**kwargs)
        for x, value_range in read_images(files, size, gpu_decode, device, batch_size, filter=filter):
            bank.value_range = value_range
            bank.add(x)
        return bank


def check_comparable(sig_a, sig_b, what):
    """ValueError naming the entries in which two ``SpectrumBank.signature()`` dictionaries differ."""
    differ = [f"{k} {sig_a[k]} / {sig_b[k]}" for k in sig_a if sig_a[k] != sig_b[k]]
    if differ:
        raise ValueError(f"{what}: the two sides must share image size, window and value-range mapping; they differ in " + ", ".join(differ))


def compare(bank_a, bank_b):
    """SpectrumResult of two ``SpectrumBank``s of any two image counts, over bins 1 .. M // 2 (fields as float64 numpy arrays and Python
    numbers; the one host synchronisation of the metric).  ValueError unless the banks share ``signature()``."""
    check_comparable(bank_a.signature(), bank_b.signature(), "compare")
    m = min(bank_a.shape)
    lo, hi = 1, m // 2
    side = []
    for bank in (bank_a, bank_b):
        cnt = bank.kept
        mean = bank.sum_db[lo:hi + 1] / cnt
        var = bank.sum_db2[lo:hi + 1] / cnt - mean * mean
        side.append((mean, torch.sqrt(torch.clamp(var, min=0.0))))
    d = side[1][0] - side[0][0]
    nb = d.shape[0]
    freq = torch.arange(lo, hi + 1, dtype=torch.float64) / m
    nan = float("nan")
    if nb:
        lsd = float(torch.sqrt(torch.mean(d * d)).item())
        t1, t2 = nb // 3, (2 * nb) // 3
        bands = tuple(float(seg.mean().item()) if seg.shape[0] else nan for seg in (d[:t1], d[t1:t2], d[t2:]))
        at = int(torch.argmax(d.abs()).item())
        peak = (float(d[at].abs().item()), float(freq[at].item()))
    else:
        lsd, bands, peak = nan, (nan, nan, nan), (nan, nan)
    host = [t.cpu().numpy() for t in (side[0][0], side[1][0], side[0][1], side[1][1])]
    return SpectrumResult(freq.numpy(), *host, lsd, bands, peak, bank_a.count, bank_b.count, bank_a.flat, bank_b.flat)


# ----------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------
def spectrum_picture(mean_a, mean_b, W):
    """(H, 2 W + 4, 3) uint8 on the planes' device: two mean spectra (H, Wh) of W-wide images, each mirrored to the full plane
    (``P[u][v] = P[-u][-v]`` for a real image), fft-shifted, log-scaled over the common range of the two and set side by side, 4 black
    columns between them."""
    def full(p):
        h, wh = p.shape
        out = torch.empty(h, W, dtype=p.dtype, device=p.device)
        out[:, :wh] = p
        if W > wh:
            v = torch.arange(wh, W, device=p.device)
            u = (-torch.arange(h, device=p.device)) % h
            out[:, wh:] = p[u][:, W - v]
        return torch.roll(out, (h // 2, W // 2), (0, 1))
    tiny = torch.finfo(torch.float64).tiny
    logs = [torch.log10(torch.clamp(full(p), min=tiny)) for p in (mean_a, mean_b)]
    finite = torch.cat([l[l > math.log10(tiny)] for l in logs])
    lo, hi = (finite.min(), finite.max()) if finite.numel() else (logs[0].min(), logs[0].max())
    span = torch.clamp(hi - lo, min=1e-300)
    grey = [torch.round(torch.clamp((l - lo) / span, 0.0, 1.0) * 255.0).to(torch.uint8) for l in logs]
    gap = torch.zeros(grey[0].shape[0], 4, dtype=torch.uint8, device=grey[0].device)
    return torch.cat([grey[0], gap, grey[1]], 1)[:, :, None].expand(-1, -1, 3).contiguous()


def write_mean_spectra(path, bank_a, bank_b):
    """The picture of ``spectrum_picture`` for two banks built with ``keep_mean_spectrum``, as one 8-bit PNG through ``GPUPngEncoder``."""
    from .png_enc import GPUPngEncoder
    pic = spectrum_picture(bank_a.mean_spectrum(), bank_b.mean_spectrum(), bank_a.shape[1])
    enc = GPUPngEncoder(device=pic.device)
    try:
        enc.save_batch(pic[None], [path])
    finally:
        enc.close()


def spectrum_of_dirs(dir_a, dir_b, size=None, filter=None, window="none", gpu_decode=False, device="cuda:0", mean_spectrum=False):
    """(SpectrumResult, bank_a, bank_b) of the .jpg / .png files of two directories; images are resized only with ``size`` (otherwise all
    must have one size), ``filter`` as in ``wu.swd``."""
    banks = [SpectrumBank.from_dir(d, size, filter, gpu_decode, device, window=window, keep_mean_spectrum=mean_spectrum)
             for d in (dir_a, dir_b)]
    return compare(*banks), banks[0], banks[1]


def format_line(r):
    return (f"Spectrum: lsd {r.lsd:.4f} dB, bands low {r.bands[0]:+.4f} mid {r.bands[1]:+.4f} high {r.bands[2]:+.4f} dB, peak {r.peak[0]:.4f} dB "
            f"at {r.peak[1]:.4f} cycles/pixel, images {r.count_a} against {r.count_b}, flat {r.flat_a} / {r.flat_b}")


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="python -m wu.spectrum", description="radial power spectrum of two directories of images: log-spectral "
                                 "distance, low / middle / high band differences (dB, B minus A) and the largest single-bin difference")
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--size", type=int, default=None, help="resize every image to SIZE x SIZE first (otherwise all must have one size)")
    ap.add_argument("--filter", default=None, choices=["box", "bilinear", "bicubic", "lanczos"],
                    help="with --size: resize with this Pillow filter (Image.resize, 8-bit) through wu.resample; absent: the training "
                         "pipeline's bilinear resize")
    ap.add_argument("--window", default="none", choices=list(WINDOWS))
    ap.add_argument("--gpu-decode", action="store_true", help="read the JPEG files through wu.jpeg.GPUJpegDecoder")
    ap.add_argument("--json", default=None, help="write frequencies, mean and standard deviation (dB) of both sides and the summary here")
    ap.add_argument("--mean-spectrum", default=None, help="write the two log-scaled, fft-shifted mean 2-D spectra side by side as an 8-bit PNG")
    args = ap.parse_args(argv)
    if args.filter is not None and not args.size:
        ap.error("--filter chooses how --size resizes: give --size")
    r, bank_a, bank_b = spectrum_of_dirs(args.dir_a, args.dir_b, args.size, args.filter, args.window, args.gpu_decode,
                                         mean_spectrum=args.mean_spectrum is not None)
    print(format_line(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"freq": r.freq.tolist(), "mean_db_a": r.mean_db_a.tolist(), "mean_db_b": r.mean_db_b.tolist(),
                       "std_db_a": r.std_db_a.tolist(), "std_db_b": r.std_db_b.tolist(), "lsd": r.lsd, "bands": list(r.bands),
                       "peak": list(r.peak), "count_a": r.count_a, "count_b": r.count_b, "flat_a": r.flat_a, "flat_b": r.flat_b,
                       "window": args.window, "image size": list(bank_a.shape)}, f)
    if args.mean_spectrum:
        write_mean_spectra(args.mean_spectrum, bank_a, bank_b)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
