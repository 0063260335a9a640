"""The oracle and the plan mirror of tests/test_gpu_wgrad_exact.py, checked without a GPU for EVERY case that file runs: the worst-case
sum stays below 2^24 (in units of 2^-10 under a bf16 LeakyReLU gate), the fp32 reference equals the float64 one and autograd's, the plan
features each case was written for hold in the mirror of csrc/conv3x3_wgrad.hip, the reference contains what makes a wrong kernel visible
(non-zero entries in every tap, zeros / positives / negatives in the gate, a non-zero bias gradient), and the operands can SEE a wrong
border rule: a weight gradient computed with the row below / the column right of the image taken from the next row of memory differs."""
import pytest
import torch
import torch.nn.functional as F

import _pointwise_ref as PR
import _wgrad_ref as R

SMALL = R.gate_cases(R.RELU)


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_wgrad_cases(c):
    p, r = R.check_features(c)
    assert R.bound(c) < R.TWO24
    assert 2 * c.n * p.ho * p.wo + 8 == R.bound(c)
    x, dy, y = R.operands(c)
    assert float(x.abs().max()) == R.RX and float(dy.abs().max()) == R.RDY
    dw, db = R.reference(c)
    dw64, db64 = R.dw_db(x, dy, c, torch.float64)
    assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)
    assert float(dw.abs().max()) + R.ACCUM <= R.bound(c) and bool((dw == dw.round()).all())
    terms = R.tap_terms(c)
    assert float(terms[1, 1]) == c.n * p.ho * p.wo and (bool((terms > 0).all()) or min(c.h, c.w) <= 2)
    for t in range(9):          # every tap that has a pixel at all, the corner taps among them
        assert (int((dw[:, :, t // 3, t % 3] != 0).sum()) > 0) == (float(terms[t // 3, t % 3]) > 0), f"{c.name}: tap {t} of the reference is all zero"
    assert int((db != 0).sum()) > 0
    assert dw.shape == (c.cout, c.cin, 3, 3) and db.shape == (c.cout,)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_wgrad_oracle_is_autograd(c):
    """conv2d_weight at both strides, odd and even sizes, equals autograd of F.conv2d in float64 (integers: exactly)."""
    x, dy, _ = R.operands(c)
    w = torch.zeros((c.cout, c.cin, 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((c.cout,), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, stride=c.stride, padding=1).backward(dy.double())
    dw, db = R.reference(c)
    assert torch.equal(w.grad, dw.double()) and torch.equal(b.grad, db.double())


@pytest.mark.parametrize("act", [R.RELU, R.LEAKY], ids=["relu", "leaky"])
def test_gated_wgrad_cases(act):
    seen = set()
    for c in R.gate_cases(act):
        p, _ = R.check_features(c)
        assert R.bound(c, act) < R.TWO24, c.name
        if act == R.LEAKY:
            assert c.dtype == "bf16" and c.n * p.ho * p.wo < 8192
        x, dy, y = R.operands(c)
        assert int((y == 0).sum()) > 0 and int((y > 0).sum()) > 0 and int((y < 0).sum()) > 0, c.name
        g = R.gated(dy, y, act, c.dtype)
        unit = R.LEAKY_BF16_UNIT if act == R.LEAKY else 1.0
        assert bool(((g / unit) == (g / unit).round()).all())
        dw, db = R.reference(c, act)
        dw64, db64 = R.dw_db(x, g, c, torch.float64)
        assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)
        assert float(dw64.abs().max()) / unit + R.ACCUM / unit <= R.bound(c, act)
        if c.n * p.ho * p.wo > 1:
            assert not torch.equal(dw, R.reference(c)[0]), f"{c.name}: the gate does not show in the reference"
        terms = R.tap_terms(c)
        for t in range(9):
            assert (int((dw[:, :, t // 3, t % 3] != 0).sum()) > 0) == (float(terms[t // 3, t % 3]) > 0), f"{c.name}: tap {t}"
        assert int((db != 0).sum()) > 0
        seen.add((R.INSTANCE[(c.dtype, c.stride)], p.TW))
    insts = [i for (d, _), i in R.INSTANCE.items() if act == R.RELU or d == "bf16"]
    for inst in insts:          # at least one case per tile width of every instance
        want = {4, 8, 16} if inst.endswith("1,256>") else {4, 8, 16, 32}
        assert {tw for i, tw in seen if i == inst} >= want, (inst, seen)


def test_leaky_bf16_gate_is_a_multiple_of_two_to_the_minus_ten():
    for v in (1.0, 2.0):
        r = (torch.tensor(v) * R.SLOPE).bfloat16().float().item()
        assert r * 1024 == round(r * 1024)
    assert (torch.tensor(1.0) * R.SLOPE).bfloat16().float().item() == 205 / 1024
    assert (torch.tensor(-1.0) * R.SLOPE).bfloat16().float().item() == -205 / 1024


def test_fp32_leaky_bound_is_meaningful():
    """The derived bound of the one comparison that is not a torch.equal: below half the smallest non-zero summand, and the fp32 CPU sum
    (another summation order of the same products) lies inside it."""
    for c in R.gate_cases(R.LEAKY, "fp32"):
        dw64, db64, bdw, bdb = R.error_bound(c, R.LEAKY)
        x, dy, y = R.operands(c)
        dw32, db32 = R.dw_db(x, R.gated(dy, y, R.LEAKY, "fp32"), c)
        assert bool(((dw32.double() - dw64).abs() <= bdw).all()) and bool(((db32.double() - db64).abs() <= bdb).all())
        # one wrong, missing or extra summand moves a sum by at least 0.2f (|x| >= 1, |dy'| >= 0.2f): the bound stays below half of that
        assert float(bdw.max()) < 0.1 and float(bdb.max()) < 0.1, c.name


def test_wgrad_table_covers_the_issue():
    tws, wprs, odd, even, empty = {}, set(), False, False, False
    for c in R.CASES:
        p, r = R.plans(c)
        tws.setdefault(R.INSTANCE[(c.dtype, c.stride)], set()).add(p.TW)
        wprs.add(r.wpr)
        odd |= any(k % 2 == 1 for k in r.group_counts)
        even |= any(k % 2 == 0 and k > 0 for k in r.group_counts)
        empty |= any(k == 0 for k in r.group_counts)
    assert tws["conv3x3_wgrad_kernel<bf16_t,2,128>"] == {4, 8, 16, 32}
    assert tws["conv3x3_wgrad_kernel<float,1,128>"] == {4, 8, 16, 32}
    assert tws["conv3x3_wgrad_kernel<float,2,64>"] == {4, 8, 16, 32}
    assert tws["conv3x3_wgrad_kernel<bf16_t,1,256>"] >= {4, 8, 16}
    assert wprs == {1, 2, 4, 8}                      # wgrad_reduce_kernel at every wpr
    assert odd and even and empty
    walks = [c for c in R.CASES if R.plans(c)[0].tps_min >= 3]
    assert {(c.dtype, c.stride) for c in walks} == {("bf16", 2), ("fp32", 2), ("fp32", 1)}
    assert all(R.plans(c)[0].tps_min != R.plans(c)[0].tps_max for c in walks)          # uneven
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    assert any(c.h % 2 == 1 and c.w % 2 == 1 for c in R.CASES if c.stride == 2)          # a last input row and column without a partner
    # the three shapes of test_conv3x3_wgrad_generic_is_exact (tests/test_gpu_conv_walk.py) give ONE tile per split; 512 -> 512 at 28 x 28, B = 16 gives 8
    for n, cin, cout, h, w in ((3, 64, 128, 40, 72), (2, 128, 64, 28, 56), (1, 64, 64, 33, 35)):
        assert R.wgrad_plan(n, cin, cout, h, w, 1, "bf16").tps_max == 1
    assert R.wgrad_plan(16, 512, 512, 28, 28, 1, "bf16").tps_min == 8


@pytest.mark.parametrize("stride", [1, 2])
def test_wrong_border_rule_is_visible(stride):
    """The mutation this suite is about: the row below an odd-height image, or the column right of an odd-width one, read as the next
    row / column of memory instead of as padding."""
    c = next(c for c in R.CASES if (c.n, c.h, c.w, c.stride, c.dtype) == (2, 13, 27, stride, "bf16"))
    assert c.h % 2 == 1 and c.w % 2 == 1
    x, dy, _ = R.operands(c)
    dw, _ = R.reference(c)
    by_hand, wrong = R.memory_order_border_dw(c, x, dy)
    assert torch.equal(by_hand, dw.double())
    assert not torch.equal(wrong, dw.double())
    diff = (wrong != dw.double())
    assert bool(diff[:, :, :, 2].any()) and bool(diff[:, :, 2, :].any()) and not bool(diff[:, :, :2, :2].any())       # the right and bottom taps, and only they


def test_act_gate_and_scatter_tables():
    for dt, shapes in R.ACT_GATE_SHAPES.items():
        e = 8 if dt == "bf16" else 4
        items = [n * h * w * c // e for n, c, h, w in shapes]
        assert items[0] < 256 and shapes[1][1] == e and items[2] > R.ACT_GATE_GRID_ITEMS and items[2] < 2 ** 31
    assert len({p for p in R.ACT_GATE_PADS}) == 3 and all(len(set(p)) == 3 for p in R.ACT_GATE_PADS[1:])
    g, y = R.act_gate_operands((2, 8, 5, 7), 1, False)
    assert torch.equal(g.bfloat16().float(), g) and int((y == 0).sum()) > 0
    lk = R.act_gate(g, y, R.LEAKY)
    assert PR.unrepresentable(lk) > 0.1          # 0.2f g needs its rounding in bf16
    names = {c.name for c in PR.S2_CASES}
    assert {c.name for c in R.S2_GATE_CASES[:2]} <= names and all(c.h % 2 == 1 and c.w % 2 == 1 for c in R.S2_GATE_CASES)
    big = R.S2_GATE_CASES[2]
    assert big.n * big.h * big.w * big.cout // 8 > R.S2_UP_GRID_ITEMS
    for c in R.S2_GATE_CASES:
        for act in (R.RELU, R.LEAKY):
            assert R.s2_gate_bound(c, act) < R.TWO24
    for v in (1.0, 2.0):
        r = (torch.tensor(v) * R.SLOPE).bfloat16().float().item()
        assert r * 1024 == round(r * 1024)
    for c in R.S2_GATE_CASES[:2]:
        ops = R.s2_gate_operands(c)
        for act in (R.RELU, R.LEAKY):
            g = R.gated(ops["dy"], ops["y"], act, "bf16")
            o = dict(w=ops["w"], dy=g)
            lin, _ = PR.s2_dgrad_reference(c, o, "ungated")
            lin64, _ = PR.s2_dgrad_reference(c, o, "ungated", torch.float64)
            assert torch.equal(lin, lin64) and float(lin.abs().max()) * (1024 if act == R.LEAKY else 1) <= R.s2_gate_bound(c, act)
            assert PR.unrepresentable(lin) > 0.01 or act == R.RELU
            assert int((ops["y"] == 0).sum()) > 0
