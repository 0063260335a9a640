"""LPIPS (Zhang et al. 2018; the ``lpips`` package with ``net='alex'``, version 0.1) and the pairwise-diversity score of multimodal
translation, on this library's HIP kernels: the AlexNet trunk on ``wu_conv_kxk_fwd`` / ``wu_pool3x3_fwd``, the scaling layer and the fused
head in csrc/lpips.hip.

    m = LPIPS()                                       # seeded random weights: see below
    m.load_alexnet(torch.load("alexnet.pth"))         # torchvision's alexnet state-dict
    m.load_lin(torch.load("alex.pth"))                # the package's linear layers
    d = m.distance(x, fakes)                          # x (B, 3, H, W), fakes (R, B, 3, H, W) as a sweep returns them -> (R, B) float64 CUDA
    p = m.pairwise(fakes)                             # (R, R, B)
    v = m.diversity(fakes)                            # (B,): the mean over i < j
    python -m wu.lpips DIR_A DIR_B --alexnet A.pth --lin L.pth

WITHOUT PRETRAINED WEIGHTS THE NUMBERS MEAN NOTHING.  Neither torchvision nor the ``lpips`` package is needed and nothing is downloaded, so a
fresh module holds seeded random values (He-normal convs, linear weights uniform in [0, 1)): enough to test the arithmetic, not a
perceptual metric.  Load torchvision's ``alexnet`` weights and the package's ``alex.pth`` before reporting anything.

Semantics, in full (tests/_lpips_ref.py restates them).  A value is widened to float32 and mapped to [-1, 1] by ``t = v * s + o``
(``value_range`` (-1, 1): s = 1, o = 0; (0, 1): s = 2, o = -1; "uint8": s = 2 / 255, o = -1), then ``u_c = (t - shift_c) / scale_c`` with
shift = (-.030, -.088, -.188), scale = (.458, .448, .450); each of the four operations is rounded to float32 on its own and the result to the
storage dtype.  Trunk: ``F_1 = relu(conv1(u))``, ``F_2 = relu(conv2(maxpool(F_1)))``, ``F_3 = relu(conv3(maxpool(F_2)))``,
``F_4 = relu(conv4(F_3))``, ``F_5 = relu(conv5(F_4))``; convs 3->64 k11 s4 p2, 64->192 k5 p2, 192->384 k3 p1, 384->256 k3 p1, 256->256 k3 p1,
all with bias; the max pool is 3 x 3, stride 2, no padding.  ``min(H, W) < 31`` raises, nothing is clamped or resized.  Head, per layer k,
on the stored features widened to float64, a = F_k(x), b = F_k(y):

    n_a = sqrt(sum_c a_c^2);  ah_c = a_c / (n_a + 1e-10)        (same for b; an all-zero vector normalises to zero)
    d_k = (1 / (h_k w_k)) sum_pixels sum_c w_kc (ah_c - bh_c)^2
    lpips(x, y) = (((d_1 + d_2) + d_3) + d_4) + d_5

No atomics, every sum in a fixed order: two runs give the same bits, and so does any ``max_images``.  CUDA tensors only: there is no CPU
fallback."""
import torch
import torch.nn as nn

from . import _lib
from .inception import conv_kxk, pool3x3, POOL_MAX
from .layout import empty_nhwc, nhwc_ld, precision_code, stream_ptr, torch_dtype

U8 = 2                                  # WU_LPIPS_U8, next to _lib.F32 / _lib.BF16
CIN0 = 16                               # the image's 3 channels, zero-padded to the conv kernel's Cin granularity
MIN_SIZE = 31
# (state-dict index, cin, cout, k, stride, pad, max pool in front)
ALEX_CONVS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True), (8, 384, 256, 3, 1, 1, False),
              (10, 256, 256, 3, 1, 1, False))
CHANNELS = tuple(c[2] for c in ALEX_CONVS)
DEFAULT_MAX_IMAGES = 64
_SRC = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: U8}


def input_mapping(value_range):
    """(s, o) of ``t = v * s + o`` as Python floats (the kernel takes them as float32)."""
    if isinstance(value_range, str):
        if value_range != "uint8":
            raise ValueError(f"value_range {value_range!r}: \"uint8\", (-1, 1) or (0, 1)")
        return 2.0 / 255.0, -1.0
    lo, hi = (float(v) for v in value_range)
    if (lo, hi) == (-1.0, 1.0):
        return 1.0, 0.0
    if (lo, hi) == (0.0, 1.0):
        return 2.0, -1.0
    raise ValueError(f"value_range {value_range}: \"uint8\", (-1, 1) or (0, 1)")


def feature_sizes(h, w):
    """[(h_k, w_k)] of the five feature maps; ValueError below 31 x 31."""
    if min(h, w) < MIN_SIZE:
        raise ValueError(f"LPIPS (alex) needs min(H, W) >= {MIN_SIZE}, got {h} x {w}; images are never clamped or resized")
    out = []
    for _, _, _, k, s, p, pool in ALEX_CONVS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((h, w))
    return out


class _Holder(nn.Module):
    """The ``features`` / ``model`` level of the state-dict names: a container whose children are numbered."""


class _Conv(nn.Module):
    def __init__(self, cin, cout, k, gen):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


def _strict_load(module, sd, what):
    own = nn.Module.state_dict(module)
    missing, unexpected = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    if missing or unexpected:
        raise RuntimeError(f"{what}: {len(missing)} missing key(s) {missing[:6]}, {len(unexpected)} unexpected key(s) {unexpected[:6]}")
    for k, v in own.items():
        if tuple(sd[k].shape) != tuple(v.shape):
            raise RuntimeError(f"{what}: {k} has shape {tuple(sd[k].shape)}, expected {tuple(v.shape)}")
    return nn.Module.load_state_dict(module, sd, strict=True)


class AlexNetFeatures(nn.Module):
    """torchvision's ``alexnet().features`` up to the last ReLU, forward-only, on HIP kernels.  Parameters are named
    ``features.{0,3,6,8,10}.{weight,bias}``; ``load_state_dict`` is strict and ignores ``classifier.*``.  ``forward(u)`` takes the NHWC
    network input (N, 16, H, W) that ``LPIPS.prepare`` makes and returns the five ReLU outputs as (N, C_k, h_k, w_k) NHWC views in the
    storage dtype.  Default weights are seeded random (He-normal, zero bias) and mean nothing."""

    def __init__(self, precision="fp32", seed=0):
        super().__init__()
        precision_code(precision)
        self.precision = precision
        gen = torch.Generator().manual_seed(seed)
        self.features = _Holder()
        for idx, cin, cout, k, _, _, _ in ALEX_CONVS:
            self.features.add_module(str(idx), _Conv(cin, cout, k, gen))
        self._plan, self._plan_key = None, None
        self.eval()

    def train(self, mode=True):
        return super().train(False)          # forward-only: always in eval mode

    def load_state_dict(self, state_dict, strict=True):
        if not strict:
            raise ValueError("AlexNetFeatures.load_state_dict is strict")
        sd = {k: v for k, v in dict(state_dict).items() if not k.startswith("classifier.")}
        return _strict_load(self, sd, "AlexNetFeatures.load_state_dict: the state-dict is not a torchvision alexnet weight set")

    def plan(self, device):
        """Packed operands of the five convs (rebuilt when a parameter's pointer or version changes)."""
        ps = list(self.parameters())
        key = (self.precision, str(device)) + tuple((p.data_ptr(), p._version) for p in ps)
        if key == self._plan_key:
            return self._plan
        code = precision_code(self.precision)
        lib = _lib.load()
        plan = []
        with torch.no_grad():
            for idx, cin_w, cout, k, s, p, pool in ALEX_CONVS:
                m = getattr(self.features, str(idx))
                cin = CIN0 if idx == 0 else cin_w
                w = m.weight.detach().float().to(device).contiguous()
                wp = torch.empty(lib.wu_conv_kxk_packed_bytes(cout, cin, k, k, code), dtype=torch.uint8, device=device)
                _lib.call("wu_pack_conv_kxk", w.data_ptr(), wp.data_ptr(), cout, cin_w, cin, k, k, code, stream_ptr())
                plan.append({"w": wp, "b": m.bias.detach().float().to(device).contiguous(), "k": (k, k), "s": (s, s), "p": (p, p),
                             "cout": cout, "cin": cin, "code": code, "pool": pool})
        self._plan, self._plan_key = plan, key
        return plan

    def forward(self, u):
        if not u.is_cuda:
            raise RuntimeError("wu.lpips: CUDA tensors only -- no CPU fallback")
        n, c, h, w = u.shape
        if c != CIN0:
            raise ValueError(f"AlexNetFeatures: the network input has {CIN0} channels (LPIPS.prepare), got {c}")
        sizes = feature_sizes(h, w)
        code = precision_code(self.precision)
        dt = torch_dtype(code)
        outs, t = [], u
        for p, (ho, wo) in zip(self.plan(u.device), sizes):
            if p["pool"]:
                hp, wp = (t.shape[2] - 3) // 2 + 1, (t.shape[3] - 3) // 2 + 1
                t = pool3x3(t, empty_nhwc(n, t.shape[1], hp, wp, dt, u.device), 2, 0, POOL_MAX, code)
            t = conv_kxk(t, p, empty_nhwc(n, p["cout"], ho, wo, dt, u.device))
            outs.append(t)
        return outs


class _Lin(nn.Module):
    """The package's NetLinLayer: ``model.1`` is the 1 x 1 conv without bias (``model.0`` is its Dropout)."""

    def __init__(self, c, gen):
        super().__init__()
        self.model = _Holder()
        conv = nn.Module()
        conv.weight = nn.Parameter(torch.rand(1, c, 1, 1, generator=gen), requires_grad=False)
        self.model.add_module("1", conv)


def head(fx, fy, weight, out, ldo=None):
    """wu_lpips_head on feature maps: fx (B, C, h, w), fy (R, B, C, h, w), NHWC storage (channel slices allowed), ``weight`` (C,) fp32;
    writes out[r * ldo + b] (float64) and returns ``out``."""
    r, b, c, h, w = fy.shape
    if tuple(fx.shape) != (b, c, h, w) or fx.dtype != fy.dtype:
        raise ValueError(f"lpips.head: fx {tuple(fx.shape)} {fx.dtype} against fy {tuple(fy.shape)} {fy.dtype}")
    lib = _lib.load()
    nbytes = lib.wu_lpips_workspace_bytes(b, r, h, w, 0)
    if nbytes == 0:
        raise ValueError(f"lpips.head: B {b} R {r} h {h} w {w} out of the kernel's range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=fx.device)
    _lib.call("wu_lpips_head", fx.data_ptr(), nhwc_ld(fx), fy.data_ptr(), nhwc_ld(fy[0]), fy.stride(0), weight.data_ptr(),
              _SRC[fx.dtype], b, r, h, w, c, ws.data_ptr(), out.data_ptr(), b if ldo is None else ldo, stream_ptr())
    return out


def pairs(f, weight, out, ldo=None):
    """wu_lpips_pairs on feature maps f (R, B, C, h, w): writes out[(i * R + j) * ldo + b] (float64) and returns ``out``."""
    r, b, c, h, w = f.shape
    lib = _lib.load()
    nbytes = lib.wu_lpips_workspace_bytes(b, r, h, w, 1)
    if nbytes == 0:
        raise ValueError(f"lpips.pairs: B {b} R {r} h {h} w {w} out of the kernel's range (2 <= R <= 64)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
    _lib.call("wu_lpips_pairs", f.data_ptr(), nhwc_ld(f[0]), f.stride(0), weight.data_ptr(), _SRC[f.dtype], b, r, h, w, c,
              ws.data_ptr(), out.data_ptr(), b if ldo is None else ldo, stream_ptr())
    return out


class LPIPS(nn.Module):
    """The metric: ``net`` (an ``AlexNetFeatures``) and the linear layers ``lin0`` .. ``lin4`` (keys ``lin{k}.model.1.weight`` of shape
    (1, C_k, 1, 1), as the package's ``alex.pth`` names them).  Default weights are seeded random and mean nothing: load both weight sets
    (``load_alexnet``, ``load_lin``) before reporting a number."""

    def __init__(self, precision="fp32", seed=0):
        super().__init__()
        precision_code(precision)
        self.precision = precision
        self.net = AlexNetFeatures(precision, seed)
        gen = torch.Generator().manual_seed(seed + 1)
        for k, c in enumerate(CHANNELS):
            self.add_module(f"lin{k}", _Lin(c, gen))
        self._lin, self._lin_key = None, None
        self.eval()

    def train(self, mode=True):
        return super().train(False)

    def load_alexnet(self, state_dict):
        return self.net.load_state_dict(state_dict)

    def load_lin(self, state_dict):
        """Strict: exactly the five ``lin{k}.model.1.weight`` keys of shape (1, C_k, 1, 1)."""
        sd = dict(state_dict)
        own = {f"lin{k}.model.1.weight": getattr(self, f"lin{k}").model.get_submodule("1").weight for k in range(5)}
        missing, unexpected = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
        if missing or unexpected:
            raise RuntimeError(f"LPIPS.load_lin: {len(missing)} missing key(s) {missing[:6]}, {len(unexpected)} unexpected key(s) "
                               f"{unexpected[:6]}")
        for k, p in own.items():
            if tuple(sd[k].shape) != tuple(p.shape):
                raise RuntimeError(f"LPIPS.load_lin: {k} has shape {tuple(sd[k].shape)}, expected {tuple(p.shape)}")
        with torch.no_grad():
            for k, p in own.items():
                p.copy_(sd[k])

    def lin_weights(self, device):
        ps = [getattr(self, f"lin{k}").model.get_submodule("1").weight for k in range(5)]
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._lin_key:
            self._lin = [p.detach().float().reshape(-1).to(device).contiguous() for p in ps]
            self._lin_key = key
        return self._lin

    # ---- input ----
    def prepare(self, images, value_range=(-1, 1), out=None):
        """(N, 3, H, W) float32 / bfloat16 / uint8 CUDA images of any strides -> the NHWC network input (N, 16, H, W) in the storage dtype
        (written into ``out``, a dense NHWC buffer of that shape, when given): one pass over the source, no intermediate copy."""
        if not (torch.is_tensor(images) and images.is_cuda):
            raise RuntimeError("wu.lpips: CUDA tensors only -- no CPU fallback")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"wu.lpips: images must be (N, 3, H, W), got {tuple(images.shape)}")
        if images.dtype not in _SRC:
            raise ValueError(f"wu.lpips: float32, bfloat16 or uint8 images, got {images.dtype}")
        n, _, h, w = images.shape
        feature_sizes(h, w)
        s, o = input_mapping(value_range)
        code = precision_code(self.precision)
        u = empty_nhwc(n, CIN0, h, w, torch_dtype(code), images.device) if out is None else out
        images = images.detach()
        _lib.call("wu_lpips_input", images.data_ptr(), *images.stride(), _SRC[images.dtype], n, h, w, s, o, u.data_ptr(), code, stream_ptr())
        return u

    def features(self, images, value_range=(-1, 1)):
        """The five feature maps of (N, 3, H, W) images."""
        return self.net(self.prepare(images, value_range))

    def features_of_rows(self, rows, value_range=(-1, 1)):
        """The five feature maps of (R, N, 3, H, W) images (any strides: a block of a sweep's output) as (R, N, C_k, h_k, w_k) views: every
        row is scaled straight into its part of one network input, the trunk runs once over the R N images."""
        nr, nb, _, h, w = rows.shape
        code = precision_code(self.precision)
        u = empty_nhwc(nr * nb, CIN0, h, w, torch_dtype(code), rows.device)
        for i in range(nr):
            self.prepare(rows[i], value_range, out=u[i * nb:(i + 1) * nb])
        return [self._rows(f, nr, nb) for f in self.net(u)]

    # ---- the metric ----
    @staticmethod
    def _total(layers):
        return (((layers[0] + layers[1]) + layers[2]) + layers[3]) + layers[4]

    def _check(self, x, fakes):
        if not (torch.is_tensor(fakes) and fakes.is_cuda and (x is None or (torch.is_tensor(x) and x.is_cuda))):
            raise RuntimeError("wu.lpips: CUDA tensors only -- no CPU fallback")
        if fakes.dim() != 5 or fakes.shape[2] != 3 or (x is not None and tuple(x.shape) != tuple(fakes.shape[1:])):
            raise ValueError(f"wu.lpips: x (B, 3, H, W) and fakes (R, B, 3, H, W), got {None if x is None else tuple(x.shape)} / "
                             f"{tuple(fakes.shape)}")
        feature_sizes(*fakes.shape[-2:])

    @torch.no_grad()
    def distance(self, x, fakes, value_range=(-1, 1), layers=False, max_images=DEFAULT_MAX_IMAGES):
        """lpips(x[b], fakes[r, b]): (R, B) float64 CUDA, or (B,) when ``fakes`` has no leading R; with ``layers=True`` also the five d_k as
        (R, B, 5).  The trunk runs over at most ``max_images`` images per pass and the head is applied per pass, so the feature maps of a
        whole sweep never exist at once.  Nothing is synchronised."""
        squeeze = torch.is_tensor(fakes) and fakes.dim() == 4
        if squeeze:
            fakes = fakes.unsqueeze(0)
        self._check(x, fakes)
        r, b = fakes.shape[:2]
        mi = max(1, int(max_images))
        dev = x.device
        lin = self.lin_weights(dev)
        out = torch.empty(5, r, b, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            for b0 in range(0, b, mi):
                nb = min(mi, b - b0)
                fx = self.features(x[b0:b0 + nb], value_range)
                rows = max(1, mi // nb)
                for r0 in range(0, r, rows):
                    nr = min(rows, r - r0)
                    fy = self.features_of_rows(fakes[r0:r0 + nr, b0:b0 + nb], value_range)
                    for k in range(5):
                        head(fx[k], fy[k], lin[k], out[k, r0:, b0:], ldo=b)
        per = out.permute(1, 2, 0)
        total = self._total(out)
        if squeeze:
            total, per = total[0], per[0]
        return (total, per) if layers else total

    @staticmethod
    def _rows(f, nr, nb):
        """(nr * nb, C, h, w) NHWC -> (nr, nb, C, h, w) with the same storage."""
        n, c, h, w = f.shape
        return f.as_strided((nr, nb, c, h, w), (nb * f.stride(0),) + tuple(f.stride()))

    @torch.no_grad()
    def pairwise(self, fakes, value_range=(-1, 1), layers=False, max_images=DEFAULT_MAX_IMAGES):
        """lpips(fakes[i, b], fakes[j, b]): (R, R, B) float64 CUDA with exact zeros on the diagonal and entry (j, i) a copy of entry (i, j);
        with ``layers=True`` also the five layer matrices (R, R, B, 5).  A pass of the trunk holds one image of every row at the least:
        max(1, max_images // R) images of each of the R rows."""
        self._check(None, fakes)
        r, b = fakes.shape[:2]
        if r < 2:
            raise ValueError(f"wu.lpips.pairwise: needs R >= 2 rows, got {r}")
        dev = fakes.device
        lin = self.lin_weights(dev)
        out = torch.empty(5, r, r, b, dtype=torch.float64, device=dev)
        step = max(1, int(max_images) // r)
        with torch.cuda.device(dev):
            for b0 in range(0, b, step):
                nb = min(step, b - b0)
                f = self.features_of_rows(fakes[:, b0:b0 + nb], value_range)
                for k in range(5):
                    pairs(f[k], lin[k], out[k, :, :, b0:], ldo=b)
        total = self._total(out)
        return (total, out.permute(1, 2, 3, 0)) if layers else total

    def diversity(self, fakes, value_range=(-1, 1), max_images=DEFAULT_MAX_IMAGES):
        """The diversity score of multimodal translation: per image, the mean of lpips(fakes[i], fakes[j]) over i < j -> (B,) float64."""
        m = self.pairwise(fakes, value_range, max_images=max_images)
        r = m.shape[0]
        iu = torch.triu_indices(r, r, 1, device=m.device)
        return m[iu[0], iu[1]].sum(0) / (r * (r - 1) // 2)


# ----------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------
def distance_of_dirs(model, dir_a, dir_b, batch_size=32, device="cuda:0"):
    """The mean LPIPS and the per-layer means over the files of two directories paired by stem (``wu.files.paired_batches``; Pillow,
    uint8 RGB; pairs batched by size): {"lpips", "layers", "pairs"}."""
    from .files import paired_batches
    sums, count = None, 0
    for xa, xb in paired_batches(dir_a, dir_b, batch_size, device):
        d, per = model.distance(xa, xb, "uint8", layers=True, max_images=batch_size)
        part = torch.cat([d.sum(0, keepdim=True), per.sum(0)])
        sums = part if sums is None else sums + part
        count += d.shape[0]
    vals = (sums / count).tolist()
    return {"lpips": vals[0], "layers": vals[1:], "pairs": count}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wu.lpips", description="LPIPS (alex, v0.1) of two directories paired by file stem")
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--alexnet", required=True, help="torchvision alexnet state-dict (torch.save)")
    ap.add_argument("--lin", required=True, help="the lpips package's alex.pth (lin{k}.model.1.weight)")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args(argv)
    model = LPIPS(args.precision)
    model.load_alexnet(torch.load(args.alexnet, map_location="cpu"))
    model.load_lin(torch.load(args.lin, map_location="cpu"))
    r = distance_of_dirs(model, args.dir_a, args.dir_b, args.batch_size)
    print(f"LPIPS: {r['lpips']:.6f}")
    print("layers: " + " ".join(f"{v:.6f}" for v in r["layers"]))
    print(f"pairs: {r['pairs']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
