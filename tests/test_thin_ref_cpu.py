"""The oracle of tests/test_gpu_thin_exact.py is not its own reference: on random REAL inputs its fp64 form equals torch autograd; its
integer premise holds for every case table; its dispatch restatement names the kernel each case was written for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _thin_cases as C
import _thin_ref as R


def _real(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(tuple(shape), generator=g, dtype=torch.float64) * 2 - 1


def _act(v, act):
    return {R.NONE: v, R.RELU: F.relu(v), R.LEAKY: F.leaky_relu(v, 0.2)}[act]


@pytest.mark.parametrize("act", [R.NONE, R.RELU, R.LEAKY])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cfg", [(2, 3, 5, 7), (1, 64, 6, 8), (3, 3, 4, 5), (1, 2, 7, 6), (2, 64, 1, 1)], ids=str)
def test_conv_oracle_equals_autograd(cfg, stride, act):
    """conv_fwd / conv_wgrad / conv_dgrad against autograd of F.conv2d + activation in fp64: odd and even H and W, both strides, all
    three activations, with inv_sigma."""
    n, cout, h, w = cfg
    x = _real((n, 3, h, w), 1).requires_grad_(True)
    wt = _real((cout, 3, 3, 3), 2)
    b = _real((cout,), 3)
    for isg in (None, 0.37):
        weff = (wt * (1.0 if isg is None else isg)).detach().requires_grad_(True)
        x.grad = None
        ref = _act(F.conv2d(x, weff, b, stride=stride, padding=1), act)
        dy = _real(ref.shape, 4)
        ref.backward(dy)
        y, bits = R.conv_fwd(x.detach(), wt, b, isg, stride, act, real=True)
        assert y.dtype == torch.float64 and (y - ref.detach()).abs().max().item() <= 1e-12
        assert torch.equal(bits, ref.detach() > 0)
        dw, db = R.conv_wgrad(x.detach(), dy, y, act, stride, real=True)
        assert (dw - weff.grad).abs().max().item() <= 1e-12
        assert (db - _grad_of_bias(x.detach(), weff.detach(), b, stride, act, dy)).abs().max().item() <= 1e-12
        dx = R.conv_dgrad(dy, y, act, wt, isg, stride, h, w, real=True)
        assert dx.shape == x.shape and (dx - x.grad).abs().max().item() <= 1e-12
        # ungated: y = None
        dwu, dbu = R.conv_wgrad(x.detach(), dy, None, R.NONE, stride, real=True)
        dwn, _ = R.conv_wgrad(x.detach(), dy, y, R.NONE, stride, real=True)
        assert torch.equal(dwu, dwn) and (dbu - dy.sum(dim=(0, 2, 3))).abs().max().item() <= 1e-12


def _grad_of_bias(x, weff, b, stride, act, dy):
    bb = b.clone().requires_grad_(True)
    _act(F.conv2d(x, weff, bb, stride=stride, padding=1), act).backward(dy)
    return bb.grad


@pytest.mark.parametrize("gate", [R.NONE, R.RELU])
@pytest.mark.parametrize("cfg", [(1, 64, 1, 1), (2, 64, 3, 5), (3, 16, 4, 2)], ids=str)
def test_head_oracle_equals_autograd(cfg, gate):
    n, cin, h, w = cfg
    x0 = _real((n, cin, h, w), 11).requires_grad_(True)
    wt = _real((3, cin), 12).requires_grad_(True)
    b = _real((3,), 13).requires_grad_(True)
    x = F.relu(x0) if gate == R.RELU else x0
    out = torch.tanh(F.conv2d(x, wt.view(3, cin, 1, 1), b))
    dout = _real(out.shape, 14)
    out.backward(dout)
    dx, dw, db = R.tanh_head_bwd(dout, out.detach(), x.detach(), wt.detach(), gate, real=True)
    assert (dx - x0.grad).abs().max().item() <= 1e-12
    assert (dw - wt.grad).abs().max().item() <= 1e-12
    assert (db - b.grad).abs().max().item() <= 1e-12


def test_leaky_gate_is_exact_on_multiples_of_five():
    """float32(0.2) * 5k rounds to k: a Leaky gate keeps integer gradients integer, in fp32 and after re-rounding to bf16."""
    k = np.arange(-400, 401, dtype=np.float32)
    assert np.array_equal(np.float32(0.2) * (np.float32(5) * k), k)
    g = torch.arange(-10, 11, 5).float()
    got = R.act_gate(g, -torch.ones_like(g), R.LEAKY)
    assert torch.equal(got, (g / 5).double()) and torch.equal(got.float().bfloat16().double(), got)
    # an exact zero is ON the closed side of the gate (y > 0 is false there): real inputs never land on it, integers do
    zero = torch.zeros_like(g)
    assert torch.equal(R.act_gate(g, zero, R.RELU), zero.double()) and torch.equal(R.act_gate(g, zero, R.LEAKY), (g / 5).double())
    assert torch.equal(R.act_gate(g, zero + 1, R.RELU), g.double()) and torch.equal(R.act_gate(g, zero, R.NONE), g.double())
    assert torch.equal(R.act_apply(zero.double(), R.LEAKY), zero) and torch.equal(R.act_apply(-g.abs().double(), R.RELU), zero)


def test_integer_forward_is_exact_in_every_format():
    """The premise on a real case: integer operands give a pre-activation that fp32 holds exactly and outputs whose bf16 rounding the
    oracle states (round to nearest even of the one fp32 LeakyReLU multiply)."""
    n, h, w = 2, 9, 11
    x = R.ints((n, 3, h, w), -C.XMAX, C.XMAX, 1)
    wt = R.ints((64, 3, 3, 3), -C.WMAX, C.WMAX, 2)
    b = R.ints((64,), -C.BMAX, C.BMAX, 3)
    y, bits = R.conv_fwd(x, wt, b, 2.0, 1, R.LEAKY)
    assert y.dtype == torch.float32 and float(y.abs().max()) <= C.fwd_bound()
    assert torch.equal(F.leaky_relu(F.conv2d(x, wt * 2, b, padding=1), 0.2), y)          # torch's fp32 conv agrees bit for bit
    assert torch.equal(bits, y > 0) and int((y == 0).sum()) > 0                          # exact zeros sit on the gate
    assert not torch.equal(y.bfloat16().float(), y)                                      # 0.2f * v: the bf16 rounding is exercised
    with pytest.raises(AssertionError):
        R.conv_fwd(x + 0.1, wt / 3, b, None, 1, R.NONE)                                  # non-integers are refused, not rounded


def test_every_case_keeps_the_integer_premise():
    R.exact(C.fwd_bound())
    for s, st, *_ in C.WGRAD_MFMA + C.WGRAD_GENERIC + C.IMG3_WGRAD + C.WGRAD_SMALL:
        for gmax in (C.GMAX, C.GMAX_LEAKY):
            xm = C.wgrad_xmax(s, st, gmax)
            assert xm >= 1
            R.exact(C.wgrad_bound(s, st, gmax, xm))
    assert C.wgrad_xmax(C.L["L1"][0], 1, C.GMAX_LEAKY) == 2 and C.wgrad_xmax(C.L["L1"][0], 1, C.GMAX) == 4      # narrowed only where needed
    for cout in (3, 32, 64):
        R.exact(C.dgrad_bound(cout, C.GMAX_LEAKY))
    for s in C.HEAD_BWD_SHAPES:
        R.exact(C.head_bwd_bound(s))
    with pytest.raises(AssertionError):
        R.exact(2 ** 24)


def _lead(ld):
    """The channel offset of a slice in the GPU tests: 64 channels into a 192-wide buffer, 2 into a 68-wide one, 8 into a 76-wide one."""
    return {192: 64, 68: 2, 76: 8, 64: 0, 0: 0}[ld]


def test_dispatch_restatement_names_the_intended_kernel():
    for s, st, dt, rows, bmod, kernel in C.FWD64:
        assert R.fwd_kernel(dt, False, *s, 64, st, bias_mod16=bmod, c3_rows=rows) == kernel, (s, st, dt, rows, bmod)
    assert R.fwd_kernel(R.BF16, False, 1, 8, 8, 64, 1, bias_mod16=None) == "conv3x3_c3_fwd_mfma_kernel"
    for s, tiled, kf, kd in C.IMG3:
        assert R.fwd_kernel(R.F32, True, *s, 3, 1, img3_tiled=tiled) == kf
        assert R.dgrad_kernel(R.F32, True, *s, 3, 1, img3_tiled=tiled) == kd
    for s, st, dt, nchw, cout, lddy, tiled, kernel in C.WGRAD_MFMA + C.WGRAD_GENERIC + C.IMG3_WGRAD + C.WGRAD_SMALL:
        esz = 2 if dt == R.BF16 else 4
        for ym in (None, (_lead(lddy) * esz) % 16):
            got = R.wgrad_kernel(dt, nchw, *s, cout, st, dy_mod16=(_lead(lddy) * esz) % 16, lddy=lddy, y_mod16=ym, ldy=lddy, img3_tiled=tiled)
            assert got == kernel, (s, st, dt, nchw, cout, lddy, tiled, ym)
    for s, st, dt, nchw, cout, lddy, ym, ldy, kernel in C.DGRAD_S2 + C.DGRAD_NHWC + C.DGRAD_GENERIC:
        esz = 2 if dt == R.BF16 else 4
        got = R.dgrad_kernel(dt, nchw, *s, cout, st, dy_mod16=(_lead(lddy) * esz) % 16, lddy=lddy, y_mod16=ym, ldy=ldy)
        assert got == kernel, (s, st, dt, nchw, cout, lddy, ym, ldy)
    kernels = {r[-1] for t in (C.FWD64, C.WGRAD_MFMA, C.WGRAD_GENERIC, C.IMG3_WGRAD, C.WGRAD_SMALL, C.DGRAD_S2, C.DGRAD_NHWC, C.DGRAD_GENERIC) for r in t}
    kernels |= {k for r in C.IMG3 for k in r[2:]}
    assert kernels == {"conv3x3_c3_fwd_mfma_kernel", "conv3x3_c3_fwd_kernel", "conv3x3_c3_fwd_rows_kernel", "img3_conv_kernel", "img3_wgrad_kernel",
                       "conv3x3_c3_wgrad_mfma_kernel", "conv3x3_c3_wgrad_kernel", "conv3x3_c3_wgrad_small_kernel", "conv3x3_c3_dgrad_s2_mfma_kernel",
                       "conv3x3_c3_dgrad_nhwc_kernel", "conv3x3_c3_dgrad_kernel"}


def test_large_shapes_iterate_their_loops():
    """The shapes named for a loop really exceed the grid cap restated in _thin_ref.py (which follows csrc/thin.hip)."""
    for k, (s, st) in C.L.items():
        assert C.npix(s, st) > R.FWD_MFMA_LOOP_PIXELS, k
    assert C.npix(*C.L["L1"]) == 532480 and C.npix(*C.L["L1"]) % 32 == 0 and -(-C.npix(*C.L["L1"]) // 32) == 16640
    assert -(-C.npix(*C.L["L1x"]) // 32) > 2 * 16384                        # some waves run three iterations
    assert C.npix(*C.L["L2"]) == 529197 and C.npix(*C.L["L2"]) % 32 == 13
    assert C.npix(*C.L["L3"]) % 32 == 0 and R.out_hw(520, 512, 2) == (260, 256)
    assert C.npix(*C.L["L4"]) == 538704 and C.npix(*C.L["L4"]) % 32 != 0 and R.out_hw(521, 515, 2) == (261, 258)
    for k in ("L1", "L2", "L4"):
        assert 2 * R.WGRAD_MFMA_LOOP_PIXELS < C.npix(*C.L[k]) < 3 * R.WGRAD_MFMA_LOOP_PIXELS and C.npix(*C.L[k]) % R.WGRAD_MFMA_LOOP_PIXELS != 0
    assert C.npix(*C.L["L2"]) > R.ROWS_LOOP_PIXELS and C.npix(*C.L["L2"]) % 256 != 0
    assert C.npix((2, 200, 200)) > R.WGRAD_GENERIC_LOOP_PIXELS
    assert C.npix((2, 364, 364)) > R.WGRAD_SMALL_LOOP_PIXELS
    assert 3 * -(-176 // R.I3H) * -(-2048 // R.I3W) == 1056 > R.IMG3_WGRAD_LOOP_TILES
    assert C.npix((8, 520, 512)) > R.DGRAD_GENERIC_LOOP_PIXELS
    assert C.npix((2, 260, 256)) > R.DGRAD_NHWC_LOOP_GROUPS * 32
    assert C.npix((2, 130, 127)) == 33020 > R.TANH_BWD_LOOP_GROUPS * 32 and 33020 % 32 != 0 and 33020 % 16 != 0
    assert 65 * 65 > 64 * 2 * 32                                             # tanh forward: 64 workgroups x 2 groups of 256 / LP <= 32 pixels
