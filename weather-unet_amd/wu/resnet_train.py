"""A TRAINABLE ResNet-101 on this library's HIP kernels: the drop-in for ``torchvision.models.resnet101(pretrained=False, num_classes=n)``
at classifier.py:106 and estimator.py:143 (the reference's first two workflow steps, sh/train_classifier.sh / sh/train_estimator.sh,
train the classifier and the estimator from scratch in train-mode BatchNorm).

    model = resnet101(num_classes=5, precision="bf16").cuda()

* Module tree and state-dict keys are torchvision's (``num_batches_tracked`` included), children in torchvision's order
  ``conv1, bn1, relu, maxpool, layer1 .. layer4, avgpool, fc`` (estimator.py:148-153 freezes "the first 7 children" by counting;
  classifier.py:108-112 swaps ``model.fc``); ``relu`` / ``maxpool`` / ``avgpool`` hold no parameters and the forward never calls
  them -- the body runs on the HIP kernels -- but it does call ``self.fc``, so a replaced head is used.  A state dict moves
  ``strict=True`` between this module and ``ResNet101Estimator``.
* ``train()``: batch-statistics BatchNorm.  The body (stem .. global average pool) is ONE autograd node with a static kernel schedule,
  like ``ResNetFn``: the forward stores each conv's pre-BN output, the batch statistics and each BN + ReLU output in the working dtype;
  the backward runs BN backward (gated by the stored ReLU output), the pointwise / 3x3 / stem weight gradients and the data gradients.
  Running statistics and ``num_batches_tracked`` move on every train-mode forward, ``torch.no_grad()`` included (the reference's
  evaluation loops run the model in train mode under no_grad: classifier.py:152-157, estimator.py:199-204).
* ``eval()``: the folded frozen path of ``ResNet101Estimator`` (same ``plan()``, same ``ResNetFn``): bit-identical outputs on the same
  state dict.  Only data gradients flow there (as for the frozen estimator).
* Frozen parameters (``requires_grad=False``) get no weight-gradient launch, and the backward stops below the lowest block that still
  trains when the input needs no gradient (estimator.py --pre_trained: layer4 + fc; classifier.py --pre_trained: fc only -- the body
  then runs forward only).
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from . import kernels as K
from .layout import dtype_code, empty_nhwc, nhwc_ld, precision_code, require_cuda, stream_ptr, torch_dtype
from .resnet import (BN_EPS, EXPANSION, LAYERS, ResNet101Estimator, ResNetFn, _BNP, _Bottleneck, _ConvP, _chunked, _half, conv1x1,
                     maxpool3s2, maxpool3s2_bwd, stem7x7, stem7x7_dgrad)

RELU, NONE = K.ACT_RELU, K.ACT_NONE
BN_MOMENTUM = 0.1                   # nn.BatchNorm2d's default (torchvision keeps it)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _ld(t):
    return nhwc_ld(t) if t is not None else 0


# ----------------------------------------------------------------------------------------------
# launch helpers (C ABI: include/wu_kernels.h, "trainable ResNet-101")
# ----------------------------------------------------------------------------------------------
def bn_stats(x, eps=BN_EPS, momentum=BN_MOMENTUM, running_mean=None, running_var=None, num_batches_tracked=None):
    """(2, C) fp32 {mean, rstd} of the NHWC tensor x over its N*H*W rows; running statistics updated as nn.BatchNorm2d.train() does."""
    n, c, h, w = x.shape
    m, code = n * h * w, dtype_code(x)
    ws = K.workspace(_lib.load().wu_bn_stats_workspace(m, c, code), x.device)
    st = torch.empty((2, c), dtype=torch.float32, device=x.device)
    _lib.call("wu_bn_stats", x.data_ptr(), nhwc_ld(x), m, c, float(eps), float(momentum), st.data_ptr(), _ptr(running_mean), _ptr(running_var),
              _ptr(num_batches_tracked), ws.data_ptr(), ws.numel(), code, stream_ptr())
    return st


def bn_apply(x, st, gamma, beta, y, act=NONE, x2=None, st2=None, gamma2=None, beta2=None, residual=None):
    """y = act(bn(x) [+ bn'(x2) | + residual]) with the batch statistics st (/ st2)."""
    n, c, h, w = x.shape
    _lib.call("wu_bn_apply", x.data_ptr(), nhwc_ld(x), st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(x2), _ld(x2), _ptr(st2), _ptr(gamma2),
              _ptr(beta2), _ptr(residual), _ld(residual), y.data_ptr(), nhwc_ld(y), n * h * w, c, act, dtype_code(x), stream_ptr())
    return y


def bn_bwd(g, y, act, x, st, gamma, dgamma, dbeta, dx, x2=None, st2=None, gamma2=None, dgamma2=None, dbeta2=None, dx2=None, gres=None):
    """BatchNorm backward from g gated by act'(y): dgamma / dbeta (fp32, overwritten), dx [, the second branch] [, gres = the gated g]."""
    n, c, h, w = x.shape
    m, code = n * h * w, dtype_code(x)
    ws = K.workspace(_lib.load().wu_bn_bwd_workspace(m, c, code), x.device)
    _lib.call("wu_bn_bwd", g.data_ptr(), nhwc_ld(g), _ptr(y), _ld(y), act, x.data_ptr(), nhwc_ld(x), st.data_ptr(), gamma.data_ptr(),
              dgamma.data_ptr(), dbeta.data_ptr(), dx.data_ptr(), nhwc_ld(dx), _ptr(x2), _ld(x2), _ptr(st2), _ptr(gamma2), _ptr(dgamma2),
              _ptr(dbeta2), _ptr(dx2), _ld(dx2), _ptr(gres), _ld(gres), m, c, ws.data_ptr(), ws.numel(), code, stream_ptr())
    return dx


def conv1x1_wgrad(x, gy, dw, in_stride=1, accumulate=False):
    """dw (Cout, Cin[, 1, 1]) fp32 (+)= sum over the output pixels of gy (x) x[gathered with in_stride]."""
    n, cin, hin, win = x.shape
    _, cout, hc, wc = gy.shape
    ws = K.workspace(_lib.load().wu_conv1x1_wgrad_workspace(n * hc * wc, cin, cout), x.device)
    _lib.call("wu_conv1x1_wgrad", x.data_ptr(), nhwc_ld(x), gy.data_ptr(), nhwc_ld(gy), dw.data_ptr(), ws.data_ptr(), ws.numel(),
              n, hc, wc, in_stride, hin, win, cin, cout, 1 if accumulate else 0, dtype_code(x), stream_ptr())
    return dw


def stem7x7_wgrad(x_nchw, gy, dw, accumulate=False):
    """dw (64, 3, 7, 7) fp32 (+)= the weight gradient of Conv2d(3, 64, 7, stride 2, padding 3) from the fp32 NCHW image."""
    n, _, h, w = x_nchw.shape
    ws = K.workspace(_lib.load().wu_stem7x7_wgrad_workspace(n, h, w), x_nchw.device)
    _lib.call("wu_stem7x7_wgrad", x_nchw.data_ptr(), gy.data_ptr(), nhwc_ld(gy), dw.data_ptr(), ws.data_ptr(), ws.numel(), n, h, w,
              1 if accumulate else 0, dtype_code(gy), stream_ptr())
    return dw


# ----------------------------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------------------------
class ResNet101(ResNet101Estimator):
    """torchvision ResNet-101 (Bottleneck, [3, 4, 23, 3]) -> (N, num_classes) raw outputs; input (N,3,H,W) fp32 NCHW with H, W >= 32.
    Shares ``ResNet101Estimator``'s parameter holders and its eval-mode plan; adds train-mode BatchNorm and weight gradients."""

    def __init__(self, num_classes=5, precision="bf16", layers=LAYERS):
        nn.Module.__init__(self)
        self.layers_cfg = tuple(layers)
        self.conv1, self.bn1 = _ConvP(64, 3, 7), _BNP(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = 64
        for li, (planes, blocks, stride) in enumerate(layers, start=1):
            mods = []
            for b in range(blocks):
                s = stride if b == 0 else 1
                mods.append(_Bottleneck(inplanes, planes, s, b == 0 and (s != 1 or inplanes != planes * EXPANSION)))
                inplanes = planes * EXPANSION
            setattr(self, f"layer{li}", nn.Sequential(*mods))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(inplanes, num_classes)
        for p in self.parameters():
            p.requires_grad_(True)
        precision_code(precision)
        self.precision = precision
        self._plan = self._plan_key = None
        self._wts = self._wts_key = None
        self._stat_gen = 0              # train-mode forwards: the kernels move the running statistics without a _version bump
        nn.Module.train(self, True)

    def train(self, mode=True):
        return nn.Module.train(self, mode)

    def _state_key(self):
        return super()._state_key() + (self._stat_gen,)

    # ---- the conv / BN pairs of the body in a fixed order ----
    def units(self):
        """[(name, conv, bn)] in forward order: the stem, then per block conv1, conv2, conv3 [, downsample]."""
        out = [("stem", self.conv1, self.bn1)]
        for blk in self.blocks():
            out += [("c1", blk.conv1, blk.bn1), ("c2", blk.conv2, blk.bn2), ("c3", blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                out.append(("ds", blk.downsample[0], blk.downsample[1]))
        return out

    def blocks(self):
        return [blk for li in range(1, len(self.layers_cfg) + 1) for blk in getattr(self, f"layer{li}")]

    def body_params(self):
        ps = []
        for _, conv, bn in self.units():
            ps += [conv.weight, bn.weight, bn.bias]
        return ps

    def train_weights(self, code):
        """The raw conv weights in the kernels' layouts (working dtype; 3x3 packed for forward and data gradient), rebuilt whenever a conv
        weight has changed (every optimizer step)."""
        from .functional import _WEIGHT_GENERATION
        convs = [conv.weight for _, conv, _ in self.units()]
        key = (code, _WEIGHT_GENERATION[0]) + tuple((w.data_ptr(), w._version) for w in convs)
        if key == self._wts_key:
            return self._wts
        dt = torch_dtype(code)
        with torch.no_grad():
            units = self.units()
            packed = K.pack_conv3x3_multi([conv.weight for name, conv, _ in units if name == "c2"], code)
            wts, k3 = [], 0
            for name, conv, _ in units:
                w = conv.weight.detach()
                if name == "stem":
                    wts.append({"w": w.float().contiguous()})
                elif name == "c2":
                    wts.append({"w": packed[k3][0], "wd": packed[k3][1]})
                    k3 += 1
                else:
                    w2 = w.view(w.shape[0], w.shape[1])
                    wts.append({"w": w2.to(dt).contiguous(), "wt": w2.t().to(dt).contiguous()})
        self._wts, self._wts_key = wts, key
        return wts

    def forward(self, x):
        require_cuda(x, "resnet101")
        if x.shape[2] < 32 or x.shape[3] < 32:
            raise ValueError(f"resnet101: input {tuple(x.shape)} is smaller than the network's stride (32)")
        code = precision_code(self.precision)
        if not self.training:
            feat = ResNetFn.apply(x, self.plan(), code)
        else:
            self._stat_gen += 1
            params = self.body_params()
            wts = self.train_weights(code)
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
                feat = ResNetTrainFn.apply(x, self, code, wts, *params)
            else:
                with torch.no_grad():
                    feat = train_body(x, self, code, wts, False)[0]
        return self.fc(torch.flatten(feat, 1))


def resnet101(num_classes=5, precision="bf16"):
    """Drop-in for ``torchvision.models.resnet101(pretrained=False, num_classes=num_classes)`` (classifier.py:106, estimator.py:143)."""
    return ResNet101(num_classes=num_classes, precision=precision)


# ----------------------------------------------------------------------------------------------
# the body as one autograd node
# ----------------------------------------------------------------------------------------------
def _conv3x3_fwd(a, w, planes, s, out):
    if s == 1 and K.conv3x3_small_supported(a, planes):
        return K.conv3x3_small(a, _chunked(w, "w"), None, out)
    return K.conv3x3(a, w["w"], None, out, s)


def train_body(x, m, code, wts, keep):
    """Train-mode forward launches -> (feat (N, 2048) fp32, saved state or None)."""
    dt, dev = torch_dtype(code), x.device
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    n, _, h, w = x.shape

    def new(c, hh, ww):
        return empty_nhwc(n, c, hh, ww, dt, dev)

    def stats(t, bn):
        return bn_stats(t, BN_EPS, BN_MOMENTUM, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    units = m.units()
    h1, w1 = _half(h, 2), _half(w, 2)
    s_pre = stem7x7(x, wts[0]["w"], None, new(64, h1, w1), NONE, code)                   # conv1
    s_st = stats(s_pre, m.bn1)
    s_out = bn_apply(s_pre, s_st, m.bn1.weight, m.bn1.bias, new(64, h1, w1), RELU)      # bn1 + relu
    h2, w2 = _half(h1, 2), _half(w1, 2)
    amax = torch.empty(n * h2 * w2 * 64, dtype=torch.uint8, device=dev) if keep else None
    cur = maxpool3s2(s_out, new(64, h2, w2), amax)                                       # maxpool
    saved, hh, ww, u = [], h2, w2, 1
    for blk in m.blocks():
        s, planes = blk.stride, blk.conv1.weight.shape[0]
        w1_, w2_, w3_ = wts[u], wts[u + 1], wts[u + 2]
        wd_ = wts[u + 3] if blk.downsample is not None else None
        ho, wo = _half(hh, s), _half(ww, s)
        a_pre = conv1x1(cur, w1_["w"], None, new(planes, hh, ww), NONE)                 # conv1
        st1 = stats(a_pre, blk.bn1)
        a = bn_apply(a_pre, st1, blk.bn1.weight, blk.bn1.bias, new(planes, hh, ww), RELU)
        b_pre = _conv3x3_fwd(a, w2_, planes, s, new(planes, ho, wo))                     # conv2 (stride here)
        st2 = stats(b_pre, blk.bn2)
        b = bn_apply(b_pre, st2, blk.bn2.weight, blk.bn2.bias, new(planes, ho, wo), RELU)
        c_pre = conv1x1(b, w3_["w"], None, new(planes * EXPANSION, ho, wo), NONE)       # conv3
        st3 = stats(c_pre, blk.bn3)
        out = new(planes * EXPANSION, ho, wo)
        if wd_ is not None:                                                              # relu(bn3(conv3) + bn_ds(conv_ds(x)))
            d_pre = conv1x1(cur, wd_["w"], None, new(planes * EXPANSION, ho, wo), NONE, in_stride=s)
            bnd = blk.downsample[1]
            std = stats(d_pre, bnd)
            bn_apply(c_pre, st3, blk.bn3.weight, blk.bn3.bias, out, RELU, x2=d_pre, st2=std, gamma2=bnd.weight, beta2=bnd.bias)
        else:                                                                            # relu(bn3(conv3) + x)
            d_pre = std = None
            bn_apply(c_pre, st3, blk.bn3.weight, blk.bn3.bias, out, RELU, residual=cur)
        if keep:
            saved.append({"x": cur, "a_pre": a_pre, "a": a, "b_pre": b_pre, "b": b, "c_pre": c_pre, "d_pre": d_pre, "out": out,
                          "st": (st1, st2, st3, std), "u": u})
        u += 4 if wd_ is not None else 3
        cur, hh, ww = out, ho, wo
    feat = torch.empty((n, cur.shape[1]), dtype=torch.float32, device=dev)
    _lib.call("wu_sumpool_fwd", cur.data_ptr(), nhwc_ld(cur), feat.data_ptr(), n, hh, ww, cur.shape[1], code, stream_ptr())
    feat.mul_(1.0 / (hh * ww))                                                           # avgpool
    state = {"x": x, "s_pre": s_pre, "s_st": s_st, "s_out": s_out, "amax": amax, "saved": saved} if keep else None
    return feat, state


class ResNetTrainFn(Function):
    @staticmethod
    def forward(ctx, x, m, code, wts, *params):
        keep = any(ctx.needs_input_grad)
        feat, state = train_body(x, m, code, wts, keep)
        if keep:
            ctx.m, ctx.code, ctx.wts, ctx.state = m, code, wts, state
        return feat

    @staticmethod
    def backward(ctx, gfeat):
        m, code, wts, S = ctx.m, ctx.code, ctx.wts, ctx.state
        needs = ctx.needs_input_grad
        need_x, pneed = needs[0], needs[4:]
        units = m.units()
        dt, dev = torch_dtype(code), gfeat.device
        x = S["x"]
        n, _, h, w = x.shape
        grads = [None] * len(pneed)

        def new(c, hh, ww):
            return empty_nhwc(n, c, hh, ww, dt, dev)

        def pgrad(ui, k, like):
            """fp32 gradient buffer for parameter k (0 conv, 1 gamma, 2 beta) of unit ui: the returned one when it trains, else scratch."""
            i = 3 * ui + k
            t = torch.empty(like.shape, dtype=torch.float32, device=dev)
            if pneed[i]:
                grads[i] = t
            return t

        def trains(ui):
            return any(pneed[3 * ui:3 * ui + 3])
        saved = S["saved"]
        # lowest block whose parameters (or anything below them) need a gradient: the backward stops there
        if need_x or trains(0):
            lowest = -1
        else:
            lowest = next((bi for bi, sv in enumerate(saved) if any(trains(sv["u"] + j) for j in range(4 if sv["d_pre"] is not None else 3))),
                          len(saved))
        last = saved[-1]["out"]
        _, c, hh, ww = last.shape
        g = new(c, hh, ww)
        gf = (gfeat.float() * (1.0 / (hh * ww))).contiguous()
        _lib.call("wu_sumpool_bwd", gf.data_ptr(), g.data_ptr(), nhwc_ld(g), n, hh, ww, c, code, stream_ptr())
        for bi in range(len(saved) - 1, max(lowest, 0) - 1, -1):
            sv = saved[bi]
            u = sv["u"]
            blk = m.blocks()[bi]
            s = blk.stride
            st1, st2, st3, std = sv["st"]
            xin, a_pre, a, b_pre, b, c_pre, d_pre, out = (sv[k] for k in ("x", "a_pre", "a", "b_pre", "b", "c_pre", "d_pre", "out"))
            planes = a.shape[1]
            # bn3 (+ bn_ds) from the gradient of the block output, gated by its ReLU
            g_c = new(c_pre.shape[1], c_pre.shape[2], c_pre.shape[3])
            if d_pre is not None:
                bnd = blk.downsample[1]
                g_d = new(*d_pre.shape[1:])
                bn_bwd(g, out, RELU, c_pre, st3, blk.bn3.weight, pgrad(u + 2, 1, blk.bn3.weight), pgrad(u + 2, 2, blk.bn3.bias), g_c,
                       x2=d_pre, st2=std, gamma2=bnd.weight, dgamma2=pgrad(u + 3, 1, bnd.weight), dbeta2=pgrad(u + 3, 2, bnd.bias), dx2=g_d)
                gres = None
            else:
                gres = new(*out.shape[1:])
                bn_bwd(g, out, RELU, c_pre, st3, blk.bn3.weight, pgrad(u + 2, 1, blk.bn3.weight), pgrad(u + 2, 2, blk.bn3.bias), g_c, gres=gres)
            if pneed[3 * (u + 2)]:
                conv1x1_wgrad(b, g_c, pgrad(u + 2, 0, blk.conv3.weight))
            g_b = conv1x1(g_c, wts[u + 2]["wt"], None, new(planes, b.shape[2], b.shape[3]), NONE)
            g_bpre = new(planes, b.shape[2], b.shape[3])
            bn_bwd(g_b, b, RELU, b_pre, st2, blk.bn2.weight, pgrad(u + 1, 1, blk.bn2.weight), pgrad(u + 1, 2, blk.bn2.bias), g_bpre)
            if pneed[3 * (u + 1)]:
                K.conv3x3_wgrad(a, g_bpre, pgrad(u + 1, 0, blk.conv2.weight), None, stride=s)
            g_a = new(planes, a.shape[2], a.shape[3])
            w2_ = wts[u + 1]
            if s == 1 and K.conv3x3_small_supported(g_bpre, planes):
                K.conv3x3_small(g_bpre, _chunked(w2_, "wd"), None, g_a)
            elif s == 1:
                K.conv3x3(g_bpre, w2_["wd"], None, g_a)
            else:
                K.conv3x3_s2_dgrad(g_bpre, w2_["wd"], g_a)
            g_apre = new(planes, a.shape[2], a.shape[3])
            bn_bwd(g_a, a, RELU, a_pre, st1, blk.bn1.weight, pgrad(u, 1, blk.bn1.weight), pgrad(u, 2, blk.bn1.bias), g_apre)
            if pneed[3 * u]:
                conv1x1_wgrad(xin, g_apre, pgrad(u, 0, blk.conv1.weight))
            if d_pre is not None and pneed[3 * (u + 3)]:
                conv1x1_wgrad(xin, g_d, pgrad(u + 3, 0, blk.downsample[0].weight), in_stride=s)
            if bi > lowest:                     # the block input's gradient: someone below still needs it
                if d_pre is not None:
                    skip = conv1x1(g_d, wts[u + 3]["wt"], None, new(*xin.shape[1:]), NONE, out_stride=s)
                else:
                    skip = gres
                g = conv1x1(g_apre, wts[u]["wt"], None, new(*xin.shape[1:]), NONE, residual=skip)
        dx = None
        if lowest == -1:
            s_out, s_pre = S["s_out"], S["s_pre"]
            g_s = maxpool3s2_bwd(g, S["amax"], None, new(64, s_out.shape[2], s_out.shape[3]))
            g_spre = new(64, s_pre.shape[2], s_pre.shape[3])
            bn_bwd(g_s, s_out, RELU, s_pre, S["s_st"], m.bn1.weight, pgrad(0, 1, m.bn1.weight), pgrad(0, 2, m.bn1.bias), g_spre)
            if pneed[0]:
                stem7x7_wgrad(x, g_spre, pgrad(0, 0, m.conv1.weight))
            if need_x:
                dx = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
                stem7x7_dgrad(g_spre, wts[0]["w"], dx, code)
        return (dx, None, None, None) + tuple(grads)
