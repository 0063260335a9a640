"""InceptionV3 forward for FID / Inception-Score evaluation (the reference's eval/inception.py: pytorch-fid's ``InceptionV3``) on this
library's HIP kernels (csrc/inception.hip; C ABI: include/wu_kernels.h, "InceptionV3 forward").

The module tree keeps torchvision's Inception3 NAMES (``Conv2d_1a_3x3.conv.weight``, ``Mixed_5b.branch_pool.bn.running_var``, ...,
``fc.weight``) as plain parameter / buffer holders, so ``load_state_dict`` takes pytorch-fid's FID weight file
(``pt_inception-2015-12-05-*.pth``) or torchvision's ImageNet ``inception_v3`` weights unchanged; torchvision itself is not needed and
nothing is downloaded.  Every BasicConv2d (conv without bias + BatchNorm(eps 1e-3) + ReLU) is folded at plan time into one conv with an
fp32 bias and runs on ``wu_conv_kxk_fwd``; a Mixed block's branches write their channel slices of one NHWC concat buffer.

``use_fid_inception=True`` is the FID variant (pytorch-fid's FIDInceptionA / C / E_1 / E_2): average pools with count_include_pad=False,
a 3x3 MAX pool in Mixed_7c's pool branch, fc 2048 -> 1008.  ``False`` is torchvision's Inception3 (count_include_pad=True average pools
everywhere, fc 2048 -> 1000).  Forward only.
"""
import torch
import torch.nn as nn

from . import _lib
from .layout import empty_nhwc, nhwc_ld, precision_code, require_cuda, stream_ptr, torch_dtype

BN_EPS = 1e-3
CIN0 = 16                                   # the image's 3 channels, zero-padded to the conv kernel's Cin granularity
RESIZE = 299
POOL_MAX, POOL_AVG, POOL_AVG_EXCL_PAD = 0, 1, 2     # WU_POOL_*


# ----------------------------------------------------------------------------------------------
# parameter holders with torchvision's names
# ----------------------------------------------------------------------------------------------
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class _ConvW(nn.Module):
    def __init__(self, cout, cin, kh, kw):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin, kh, kw) * (2.0 / (cin * kh * kw)) ** 0.5, requires_grad=False)


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class BasicConv2d(nn.Module):
    """torchvision's BasicConv2d: ``conv`` (no bias) + ``bn`` (eps 1e-3) + ReLU."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.k, self.s, self.p = _pair(kernel_size), _pair(stride), _pair(padding)
        self.conv = _ConvW(cout, cin, *self.k)
        self.bn = _BN(cout)


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1 = BasicConv2d(cin, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, 1)
        self.branch7x7_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)


# ----------------------------------------------------------------------------------------------
# launch helpers
# ----------------------------------------------------------------------------------------------
def conv_kxk(x, p, y, act=_lib.ACT_RELU):
    """y = act(conv(x) + bias) with the packed plan entry ``p`` (wu_conv_kxk_fwd); x, y NHWC views, y may be a channel slice."""
    n, cin, h, w = x.shape
    kh, kw = p["k"]
    _lib.call("wu_conv_kxk_fwd", x.data_ptr(), nhwc_ld(x), p["w"].data_ptr(), p["b"].data_ptr(), y.data_ptr(), nhwc_ld(y),
              n, h, w, cin, p["cout"], kh, kw, p["s"][0], p["s"][1], p["p"][0], p["p"][1], act, p["code"], stream_ptr())
    return y


def pool3x3(x, y, stride, pad, mode, code):
    n, c, h, w = x.shape
    _lib.call("wu_pool3x3_fwd", x.data_ptr(), nhwc_ld(x), y.data_ptr(), nhwc_ld(y), n, h, w, c, stride, pad, mode, code, stream_ptr())
    return y


def global_avgpool(x, code):
    """(N, C, H, W) NHWC -> (N, C) fp32 spatial mean (fixed summation order)."""
    n, c, h, w = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _lib.call("wu_global_avgpool_fwd", x.data_ptr(), nhwc_ld(x), out.data_ptr(), c, n, h, w, c, code, stream_ptr())
    return out


def _out_hw(h, w, k, s, p):
    return (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1


class InceptionV3(nn.Module):
    """pytorch-fid's InceptionV3 on HIP kernels: ``forward(images)`` returns the requested blocks' outputs (N, C, h, w), sorted by index.

    Block 0: first max pool (64 ch), 1: second max pool (192), 2: Mixed_6e (768), 3: final average pool (2048, fp32, 1 x 1).  Blocks 0-2
    come in the precision's storage dtype (fp32 / bf16) as channels-last views.  ``logits(images)`` adds the fc head (fp32)."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, precision="fp32", resize="legacy"):
        super().__init__()
        if resize not in ("legacy", "clean"):
            raise ValueError(f"resize must be 'legacy' or 'clean', got {resize!r}")
        if resize == "clean" and not resize_input:
            raise ValueError("resize='clean' is a resize rule: it needs resize_input=True")
        self.resize = resize
        self._resampler = None
        if requires_grad:
            raise ValueError("InceptionV3 here is forward-only (evaluation): requires_grad=True is not supported")
        self.output_blocks = sorted(output_blocks)
        if not self.output_blocks or self.output_blocks[0] < 0 or self.output_blocks[-1] > 3:
            raise ValueError(f"output_blocks must be indices 0..3, got {output_blocks}")
        self.last_needed_block = self.output_blocks[-1]
        self.resize_input, self.normalize_input = resize_input, normalize_input
        self.use_fid_inception = use_fid_inception
        precision_code(precision)
        self.precision = precision
        self.num_classes = 1008 if use_fid_inception else 1000

        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, self.num_classes)
        for p in self.parameters():
            p.requires_grad_(False)
        self._plan, self._plan_key = None, None
        self.eval()

    def train(self, mode=True):
        return super().train(False)          # eval mode for good: BatchNorm folding relies on it

    # ---- weights ----
    def load_state_dict(self, state_dict, strict=True):
        """Strict by default.  Accepts pytorch-fid's FID weight file (use_fid_inception=True) or torchvision's ImageNet inception_v3
        state-dict (False; its ``AuxLogits.*`` entries are ignored); BatchNorm ``num_batches_tracked`` entries may be absent."""
        sd = dict(state_dict)
        if not self.use_fid_inception:
            sd = {k: v for k, v in sd.items() if not k.startswith("AuxLogits.")}
        own = super().state_dict()
        for k, v in own.items():
            if k.endswith(".num_batches_tracked") and k not in sd:
                sd[k] = v
        if strict:
            missing = sorted(set(own) - set(sd))
            unexpected = sorted(set(sd) - set(own))
            if missing or unexpected:
                variant = "pytorch-fid FID Inception (pt_inception-2015-12-05)" if self.use_fid_inception else "torchvision inception_v3"
                raise RuntimeError(f"InceptionV3.load_state_dict: the state-dict is not a {variant} weight set: "
                                   f"{len(missing)} missing key(s) {missing[:6]}, {len(unexpected)} unexpected key(s) {unexpected[:6]}")
        return super().load_state_dict(sd, strict=strict)

    def _state_key(self, device):
        ts = list(self.parameters()) + list(self.buffers())
        return (self.precision, str(device)) + tuple((t.data_ptr(), t._version) for t in ts)

    def plan(self, device):
        """Folded, packed operands of every conv (rebuilt when a parameter or buffer changes)."""
        key = self._state_key(device)
        if key == self._plan_key:
            return self._plan
        code = precision_code(self.precision)
        plan = {}
        with torch.no_grad():
            for name, mod in self.named_modules():
                if not isinstance(mod, BasicConv2d):
                    continue
                bn = mod.bn
                scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + BN_EPS)
                w = (mod.conv.weight.double() * scale.view(-1, 1, 1, 1)).float().to(device).contiguous()
                b = (bn.bias.double() - bn.running_mean.double() * scale).float().to(device).contiguous()
                plan[name] = self._pack(w, b, mod.k, mod.s, mod.p, code, CIN0 if name == "Conv2d_1a_3x3" else w.shape[1])
            # fc as a 1x1 conv over N x 1 x 1 pixels, fp32 in both precisions (its input is the fp32 pool3 feature)
            cp = (self.num_classes + 15) // 16 * 16
            w = torch.zeros(cp, 2048, 1, 1, device=device)
            w[:self.num_classes, :, 0, 0] = self.fc.weight.float().to(device)
            b = torch.zeros(cp, device=device)
            b[:self.num_classes] = self.fc.bias.float().to(device)
            plan["fc"] = self._pack(w, b, (1, 1), (1, 1), (0, 0), _lib.F32, 2048)
        self._plan, self._plan_key = plan, key
        return plan

    @staticmethod
    def _pack(w, b, k, s, p, code, cin):
        cout, cin_w = w.shape[0], w.shape[1]
        nbytes = _lib.load().wu_conv_kxk_packed_bytes(cout, cin, k[0], k[1], code)
        wp = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        _lib.call("wu_pack_conv_kxk", w.data_ptr(), wp.data_ptr(), cout, cin_w, cin, k[0], k[1], code, stream_ptr())
        return {"w": wp, "b": b, "k": k, "s": s, "p": p, "cout": cout, "cin": cin, "code": code}

    # ---- forward ----
    def _check_size(self, h, w):
        """Raise if an h x w network input cannot reach the last requested block (valid convs / pools need 3 x 3 inputs)."""
        def need3(hh, ww, where):
            if hh < 3 or ww < 3:
                raise ValueError(f"InceptionV3: a {h} x {w} input is too small to reach block {self.last_needed_block} "
                                 f"({where} sees {hh} x {ww}, needs at least 3 x 3); use resize_input=True or larger images")
        need3(h, w, "Conv2d_1a_3x3")
        h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        need3(h, w, "Conv2d_2a_3x3")
        h, w = h - 2, w - 2
        need3(h, w, "the first max pool")
        h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        if self.last_needed_block >= 1:
            need3(h, w, "Conv2d_4a_3x3")
            h, w = h - 2, w - 2
            need3(h, w, "the second max pool")
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        if self.last_needed_block >= 2:
            need3(h, w, "Mixed_6a")
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        if self.last_needed_block >= 3:
            need3(h, w, "Mixed_7a")

    def prepare(self, images, value_range=(0, 1), sizes=None):
        """Images -> the NHWC network input (N, 16, 299, 299) [or the input size without resize_input] in the storage dtype.
        ``images``: (N, 3, H, W) float32 (values in ``value_range``: (0, 1) or (-1, 1)) or (N, H, W, 3) uint8 (wu.infer_driver.to_uint8).
        ``resize="clean"``: the resize is Pillow's antialiased bicubic filter on float32 channels (wu.resample, float mode) instead of the
        aliased bilinear one; ``images`` may then be a padded ragged uint8 batch (N, Hmax, Wmax, 3) with ``sizes`` = [(h, w)] per image."""
        require_cuda(images, "InceptionV3")
        code = precision_code(self.precision)
        if self.resize == "clean":
            if self._resampler is None:
                from .resample import GPUResampler
                self._resampler = GPUResampler(RESIZE, "bicubic", "f32", "unit")
            return self._resampler.inception_input(images, sizes, value_range, CIN0, code, self.normalize_input)
        if sizes is not None:
            raise ValueError("InceptionV3: sizes (a ragged batch) need resize='clean'; the legacy resize reads one size per batch")
        if images.dtype == torch.uint8:
            if images.dim() != 4 or images.shape[3] != 3:
                raise ValueError(f"InceptionV3: uint8 images must be (N, H, W, 3), got {tuple(images.shape)}")
            images = images.contiguous()
            n, hin, win, _ = images.shape
            src_u8, scale, shift = 1, 1.0, 0.0
        elif images.dtype == torch.float32:
            if images.dim() != 4 or images.shape[1] != 3:
                raise ValueError(f"InceptionV3: float images must be (N, 3, H, W), got {tuple(images.shape)}")
            images = images.contiguous()
            n, _, hin, win = images.shape
            lo, hi = value_range
            if (lo, hi) == (0, 1):
                scale, shift = 1.0, 0.0
            elif (lo, hi) == (-1, 1):
                scale, shift = 0.5, 0.5
            else:
                raise ValueError(f"value_range must be (0, 1) or (-1, 1), got {value_range}")
            src_u8 = 0
        else:
            raise TypeError(f"InceptionV3: images must be float32 NCHW or uint8 NHWC, got {images.dtype}")
        ho, wo = (RESIZE, RESIZE) if self.resize_input else (hin, win)
        if not self.resize_input:
            self._check_size(hin, win)
        x = empty_nhwc(n, CIN0, ho, wo, torch_dtype(code), images.device)
        _lib.call("wu_inception_input", images.data_ptr(), src_u8, n, hin, win, scale, shift, 1 if self.normalize_input else 0,
                  x.data_ptr(), CIN0, ho, wo, CIN0, code, stream_ptr())
        return x

    def forward(self, images, value_range=(0, 1), sizes=None):
        x = self.prepare(images, value_range, sizes)
        return self._blocks(x, self.output_blocks, self.last_needed_block)

    def logits(self, images, value_range=(0, 1), sizes=None):
        """(N, num_classes) fp32 logits: pool3 features through ``fc`` (eval mode: no dropout)."""
        x = self.prepare(images, value_range, sizes)
        feat = self._blocks(x, [3], 3)[0]
        P = self.plan(feat.device)
        n = feat.shape[0]
        cp = P["fc"]["cout"]
        out = empty_nhwc(n, cp, 1, 1, torch.float32, feat.device)
        conv_kxk(feat, P["fc"], out, act=_lib.ACT_NONE)
        return out[:, :self.num_classes, 0, 0]

    def _blocks(self, x, want, last):
        P = self.plan(x.device)
        code = precision_code(self.precision)
        dt, dev = torch_dtype(code), x.device
        n = x.shape[0]
        fid = self.use_fid_inception
        avg_mode = POOL_AVG_EXCL_PAD if fid else POOL_AVG

        def new(c, h, w):
            return empty_nhwc(n, c, h, w, dt, dev)

        def conv(name, t, out=None):
            p = P[name]
            ho, wo = _out_hw(t.shape[2], t.shape[3], p["k"], p["s"], p["p"])
            return conv_kxk(t, p, out if out is not None else new(p["cout"], ho, wo))

        def maxpool_s2(t, out=None):
            ho, wo = (t.shape[2] - 3) // 2 + 1, (t.shape[3] - 3) // 2 + 1
            return pool3x3(t, out if out is not None else new(t.shape[1], ho, wo), 2, 0, POOL_MAX, code)

        def pool_s1(t, mode):
            return pool3x3(t, new(t.shape[1], t.shape[2], t.shape[3]), 1, 1, mode, code)

        def mixed_a(m, t):
            pf = P[m + ".branch_pool"]["cout"]
            out = new(224 + pf, t.shape[2], t.shape[3])
            conv(m + ".branch1x1", t, out[:, 0:64])
            conv(m + ".branch5x5_2", conv(m + ".branch5x5_1", t), out[:, 64:128])
            conv(m + ".branch3x3dbl_3", conv(m + ".branch3x3dbl_2", conv(m + ".branch3x3dbl_1", t)), out[:, 128:224])
            conv(m + ".branch_pool", pool_s1(t, avg_mode), out[:, 224:224 + pf])
            return out

        def mixed_b(m, t):
            c = t.shape[1]
            ho, wo = (t.shape[2] - 3) // 2 + 1, (t.shape[3] - 3) // 2 + 1
            out = new(480 + c, ho, wo)
            conv(m + ".branch3x3", t, out[:, 0:384])
            conv(m + ".branch3x3dbl_3", conv(m + ".branch3x3dbl_2", conv(m + ".branch3x3dbl_1", t)), out[:, 384:480])
            maxpool_s2(t, out[:, 480:480 + c])
            return out

        def mixed_c(m, t):
            out = new(768, t.shape[2], t.shape[3])
            conv(m + ".branch1x1", t, out[:, 0:192])
            u = conv(m + ".branch7x7_2", conv(m + ".branch7x7_1", t))
            conv(m + ".branch7x7_3", u, out[:, 192:384])
            u = conv(m + ".branch7x7dbl_4", conv(m + ".branch7x7dbl_3", conv(m + ".branch7x7dbl_2", conv(m + ".branch7x7dbl_1", t))))
            conv(m + ".branch7x7dbl_5", u, out[:, 384:576])
            conv(m + ".branch_pool", pool_s1(t, avg_mode), out[:, 576:768])
            return out

        def mixed_d(m, t):
            c = t.shape[1]
            ho, wo = (t.shape[2] - 3) // 2 + 1, (t.shape[3] - 3) // 2 + 1
            out = new(512 + c, ho, wo)
            conv(m + ".branch3x3_2", conv(m + ".branch3x3_1", t), out[:, 0:320])
            u = conv(m + ".branch7x7x3_3", conv(m + ".branch7x7x3_2", conv(m + ".branch7x7x3_1", t)))
            conv(m + ".branch7x7x3_4", u, out[:, 320:512])
            maxpool_s2(t, out[:, 512:512 + c])
            return out

        def mixed_e(m, t, pool_mode):
            out = new(2048, t.shape[2], t.shape[3])
            conv(m + ".branch1x1", t, out[:, 0:320])
            u = conv(m + ".branch3x3_1", t)
            conv(m + ".branch3x3_2a", u, out[:, 320:704])
            conv(m + ".branch3x3_2b", u, out[:, 704:1088])
            u = conv(m + ".branch3x3dbl_2", conv(m + ".branch3x3dbl_1", t))
            conv(m + ".branch3x3dbl_3a", u, out[:, 1088:1472])
            conv(m + ".branch3x3dbl_3b", u, out[:, 1472:1856])
            conv(m + ".branch_pool", pool_s1(t, pool_mode), out[:, 1856:2048])
            return out

        outs = []
        # block 0: stem to the first max pool
        x = maxpool_s2(conv("Conv2d_2b_3x3", conv("Conv2d_2a_3x3", conv("Conv2d_1a_3x3", x))))
        if 0 in want:
            outs.append(x)
        if last >= 1:
            x = maxpool_s2(conv("Conv2d_4a_3x3", conv("Conv2d_3b_1x1", x)))
            if 1 in want:
                outs.append(x)
        if last >= 2:
            for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
                x = mixed_a(m, x)
            x = mixed_b("Mixed_6a", x)
            for m in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
                x = mixed_c(m, x)
            if 2 in want:
                outs.append(x)
        if last >= 3:
            x = mixed_d("Mixed_7a", x)
            x = mixed_e("Mixed_7b", x, avg_mode)
            x = mixed_e("Mixed_7c", x, POOL_MAX if fid else POOL_AVG)
            feat = global_avgpool(x, code)                           # (N, 2048) fp32
            outs.append(feat.view(n, 1, 1, 2048).permute(0, 3, 1, 2))
        return outs
