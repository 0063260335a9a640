"""The oracle, the case tables and the plan restatements of tests/test_gpu_conv_s1_exact.py, checked without a GPU for EVERY case that file
runs: the worst-case sum stays below 2^24 (on the 2^-10 grid where a leaky bf16 mask puts the operands), the fp32 reference equals the
float64 reference exactly, the reference contains what makes a wrong kernel visible (exact zeros in front of the activation and in every
gate and mask, bf16 outputs that need rounding, negative values in front of LeakyReLU, leaky gates whose second rounding shows), and the
tables cover what they were written to cover -- collected from template_plan / small_plan, so that a later edit of a table cannot silently
drop a template instance, a branch of the ring's waits or a tile width."""
import pytest
import torch

import _conv_s1_ref as R

MIN_UNREPRESENTABLE = 0.01


def _ids(c):
    return c.name


@pytest.mark.parametrize("c", R.TEMPLATE_CASES + R.SMALL_CASES, ids=_ids)
def test_case_premises(c):
    has_b, act, gact, mact, dgrad = R.EPILOGUES[c.epi]
    bound = R.s1_bound(c)
    assert bound < R.TWO24
    ops = R.s1_operands(c)
    for k in ("x", "w", "gate", "mask"):
        assert ops[k] is None or float(ops[k].abs().max()) <= 256          # exact in bf16
    assert (ops["bias"] is not None) == has_b and (ops["gate"] is not None) == (gact != R.NONE) and (ops["mask"] is not None) == (mact != R.NONE)
    staged = R.s1_staged(c, ops)
    unit = 1024.0 if mact == R.LEAKY else 1.0
    assert torch.equal(staged * unit, (staged * unit).round())                 # the operands' grid
    assert c.dtype == "fp32" or torch.equal(staged.bfloat16().float(), staged)
    lin, pre, out = R.s1_reference(c, ops)
    lin64, pre64, out64 = R.s1_reference(c, ops, torch.float64)
    assert torch.equal(lin, lin64) and torch.equal(pre, pre64) and torch.equal(out, out64)
    assert float(lin.abs().max()) * unit <= bound
    # the worst case itself, in float64: sum |w| |x| + |bias|
    worst = torch.nn.functional.conv2d(staged.double().abs(), ops["w"].double().abs().transpose(0, 1).flip(2, 3) if dgrad else ops["w"].double().abs(), padding=1)
    assert float(worst.max() + (ops["bias"].abs().max() if has_b else 0)) * unit <= bound
    assert out.shape == (c.n, c.cout, c.h, c.w)
    if act != R.NONE:
        assert int((lin == 0).sum()) > 0, "no exact zero in front of the activation"
    if act == R.LEAKY:
        assert int((lin < 0).sum()) > 0, "no negative value in front of LeakyReLU"
    if gact != R.NONE:
        assert int((ops["gate"] == 0).sum()) > 0 and int((ops["gate"] > 0).sum()) > 0 and int((ops["gate"] < 0).sum()) > 0
    if mact != R.NONE:
        assert int((ops["mask"] == 0).sum()) > 0 and int((ops["mask"] > 0).sum()) > 0 and int((ops["mask"] < 0).sum()) > 0
    if c.dtype == "bf16":
        frac = R.unrepresentable(pre)
        assert frac >= MIN_UNREPRESENTABLE, f"only {frac:.4f} of the values in front of the rounding are not bf16 values"
        if gact == R.LEAKY:
            # the two roundings are visible: gating the fp32 value and rounding once gives other bits somewhere
            once = R.act_gate(pre, ops["gate"], gact).bfloat16()
            assert not torch.equal(once, out.bfloat16()), "one rounding and two roundings agree everywhere: the case cannot tell them apart"


def test_data_gradient_form_is_autograd():
    """The oracle of the gated cases is the gradient of F.conv2d with respect to its input."""
    c = next(c for c in R.TEMPLATE_CASES if c.epi == "gate_relu" and c.dtype == "fp32")
    ops = R.s1_operands(c)
    x = torch.zeros((c.n, c.cout, c.h, c.w), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, ops["w"].double(), padding=1).backward(ops["x"].double())
    assert torch.equal(x.grad.float(), R.s1_reference(c, ops)[0])


def test_leaky_mask_grid():
    """bf16(0.2f k) is a multiple of 2^-10 for |k| <= LEAKY_MASK_RX and at most |k|: the grid and the range s1_bound assumes."""
    k = torch.arange(-R.LEAKY_MASK_RX, R.LEAKY_MASK_RX + 1, dtype=torch.float32)
    v = (k * R.SLOPE).bfloat16().float()
    assert torch.equal(v * 1024, (v * 1024).round()) and bool((v.abs() <= k.abs()).all())
    assert (v[R.LEAKY_MASK_RX + 1:] * 1024).tolist() == [205.0, 410.0, 616.0, 820.0]


def test_template_table_covers_what_it_was_written_for():
    for dtype in ("fp32", "bf16"):
        mine = [c for c in R.TEMPLATE_CASES if c.dtype == dtype]
        plans = {c: R.template_plan(c.h, c.w, c.cin, dtype) for c in mine}
        assert {1 << p.tw_log2 for p in plans.values()} == {4, 8, 16, 32}, dtype
        for tw in (4, 8, 16, 32):
            of_tw = [(c, p) for c, p in plans.items() if 1 << p.tw_log2 == tw]
            assert any(p.tiles_y >= 2 and c.h % p.TH != 0 and c.w % tw != 0 for c, p in of_tw), (dtype, tw, "two tile rows, ragged in H and W")
            assert all(p.tiles_x == 1 for _, p in of_tw) or tw == 32          # W <= 16 is always ONE tile column
        assert any(p.tiles_y >= 2 and p.tiles_x >= 2 and c.h % p.TH != 0 and c.w % 32 != 0 for c, p in plans.items()), dtype
        assert any(c.h % p.TH == 0 and c.w % (1 << p.tw_log2) == 0 for c, p in plans.items()), (dtype, "a full tile")
        chunks = {p.nchunks for p in plans.values()}
        assert {1, 2} <= chunks and max(chunks) >= 3, (dtype, chunks)
        assert {c.cin for c in mine} >= {R.CHUNK[dtype], 2 * R.CHUNK[dtype], 3 * R.CHUNK[dtype]}
        assert {c.cout // 64 for c in mine} >= {1, 3}
        assert 1 in {c.n for c in mine} and max(c.n for c in mine) >= 3
        assert {c.epi for c in mine} == set(R.TEMPLATE_EPILOGUES[dtype]), dtype
        assert all(p.halo_pix <= 7 * 256 // 4 for p in plans.values())       # the template's staging capacity (launch_conv: NH = 7)
    assert "mask_leaky" not in R.TEMPLATE_EPILOGUES["fp32"] and "mask_leaky" in R.TEMPLATE_EPILOGUES["bf16"]
    names = [c.name for c in R.TEMPLATE_CASES + R.SMALL_CASES]
    seeds = [c.seed for c in R.TEMPLATE_CASES + R.SMALL_CASES]
    assert len(set(names)) == len(names) and len(set(seeds)) == len(seeds)


def _dispatch_of(c, opts):
    has_b, act, gact, mact, _ = R.EPILOGUES[c.epi]
    return R.dispatch(c.dtype, c.n, c.h, c.w, c.cin, c.cout, has_b, act, gact != R.NONE, mact != R.NONE, opts)


def test_every_route_to_the_template_is_used_and_is_what_it_says():
    bf = [c for c in R.TEMPLATE_CASES if c.dtype == "bf16"]
    assert {c.route for c in bf} == set(R.ROUTES) - {"fp32"}
    assert all(c.route == "fp32" for c in R.TEMPLATE_CASES if c.dtype == "fp32")
    for c in R.TEMPLATE_CASES:
        has_b, act, gact, mact, _ = R.EPILOGUES[c.epi]
        assert _dispatch_of(c, R.ROUTES[c.route]) == "template", c.name
        if c.route == "cin32":
            assert c.cin == 32 and c.w > 16 and mact == R.NONE
        elif c.route == "gate_epilogue":
            assert R.v2_eligible(c.h, c.w, c.cin, c.cout, c.dtype, False) and gact != R.NONE and (has_b or act != R.NONE)
        elif c.route == "opt0":
            assert c.w > 16 and _dispatch_of(c, {}) == "v2", c.name
        elif c.route == "opt3":
            assert c.w <= 16 and _dispatch_of(c, {}) == "small", c.name
        elif c.route == "mask":
            assert mact != R.NONE
    # every one of the three switched-off-small runs of the small cases is a template run too
    for c in R.SMALL_CASES:
        assert _dispatch_of(c, {R.OPT_CONV_SMALL: 0}) == "template" and _dispatch_of(c, {R.OPT_CONV_SMALL: 2}) == "small", c.name


def test_small_table_covers_what_it_was_written_for():
    plans = {c: R.small_plan(c.n, c.h, c.w, c.cin, c.cout) for c in R.SMALL_CASES}
    assert all(p is not None and p.nhk <= R.SMALL_MAX_NHK for p in plans.values())
    assert {R.small_instance(p) for p in plans.values()} == {(3, 3), (4, 3), (5, 2)}
    assert {p.nhk for p in plans.values()} >= {3, 4, 5}
    assert {1 << p.tw_log2 for p in plans.values()} == {4, 8, 16}
    assert {p.tiles_y for p in plans.values() if p.ipt == 1} >= {1, 2, 3}
    stacked = [(c, p) for c, p in plans.items() if p.ipt > 1]
    assert all(p.tiles_y == 1 for _, p in stacked)
    assert any(c.n % p.ipt != 0 and p.groups >= 2 for c, p in stacked), "no partly empty last group behind a full one"
    assert any(c.n < p.ipt for c, p in stacked), "no group with fewer images than one tile holds"
    assert any(R.small_rows_valid(p, c.h) < (128 >> p.tw_log2) for c, p in stacked), "no unused tile rows (the rows_valid clamp)"
    assert any(R.small_rows_valid(p, c.h) == (128 >> p.tw_log2) for c, p in stacked)
    assert any(p.ipt < (128 >> p.tw_log2) // c.h for c, p in stacked), "no stacking factor lowered by the 320-pixel cap"
    assert any(c.w % (1 << p.tw_log2) != 0 for c, p in plans.items()), "no ragged W"
    assert any(c.h % (128 >> p.tw_log2) != 0 and p.ipt == 1 and p.tiles_y >= 2 for c, p in plans.items()), "no ragged last row tile"
    d3 = {p.nchunks for p in plans.values() if p.depth == 3}
    d2 = {p.nchunks for p in plans.values() if p.depth == 2}
    assert {1, 2, 3} <= d3 and max(d3) >= 5, d3          # every branch of `younger` and the partial prologue at ring depth 3
    assert {1, 2} <= d2 and max(d2) >= 3, d2
    assert {c.epi for c in R.SMALL_CASES} == set(R.SMALL_EPILOGUES)
    assert {c.cout // 64 for c in R.SMALL_CASES} >= {1, 2, 4}
    assert all(p.depth == (3 if p.nhk <= 4 else 2) for p in plans.values())


def test_small_plan_against_the_published_facts():
    """The comments of csrc/conv3x3_small.hip and tests/test_gpu_round4.py, and the table of the issue this file answers."""
    P = R.small_plan
    assert P(5, 8, 8, 128, 64)[:2] == (3, 2) and P(5, 8, 8, 128, 64).groups == 3                    # two 8x8 images per tile
    p = P(7, 5, 3, 96, 64)
    assert (1 << p.tw_log2, p.ipt, p.groups, p.nhk, R.small_rows_valid(p, 5)) == (4, 6, 2, 4, 30)    # six 5-row images per 32-row tile, two unused rows
    p = P(40, 2, 2, 64, 64)
    assert (p.ipt, p.nhk, p.depth, p.halo_pix) == (13, 5, 2, 312)                                    # thirteen 2x2 images (the 320-pixel cap)
    assert P(2, 24, 16, 128, 128).tiles_y == 3 and P(2, 24, 16, 128, 128).ipt == 1                  # three row tiles for 24 x 16
    p = P(5, 16, 16, 256, 256)
    assert (1 << p.tw_log2, p.ipt, p.tiles_y, p.nhk, p.depth) == (16, 1, 2, 3, 3)                    # one 16x16 image = two 8-row tiles
    assert (P(1, 1, 1, 32, 64).ipt, P(1, 1, 1, 32, 64).nhk, P(1, 1, 1, 32, 64).nchunks) == (17, 5, 1)
    assert (P(3, 2, 16, 64, 64).ipt, P(3, 2, 16, 64, 64).nhk) == (4, 5)
    assert (P(2, 40, 4, 64, 64).ipt, P(2, 40, 4, 64, 64).tiles_y, P(2, 40, 4, 64, 64).nhk) == (1, 2, 4)
    assert (P(3, 8, 8, 32, 64).nhk, P(3, 8, 8, 32, 64).depth, P(3, 8, 8, 32, 64).nchunks) == (4, 3, 1)
    assert (P(9, 4, 4, 64, 64).ipt, P(9, 4, 4, 64, 64).groups) == (8, 2)                             # eight 4x4 images per tile
    assert P(1, 8, 17, 64, 64) is None and P(1, 8, 8, 48, 64) is None and P(1, 8, 8, 64, 32) is None


def test_no_shape_gives_fewer_than_three_halo_pieces():
    """conv_small_launch pads a launch with nhk < 3 up to the <3, 3> instance; no shape reaches that: an unstacked tile has 180 or 204 halo
    pixels, a stacked one at least 168.  The table therefore has no such case, and every shape up to 64 x 16 stays within five pieces."""
    seen = set()
    for h in range(1, 65):
        for w in range(1, 17):
            p = R.small_plan(1, h, w, 32, 64)
            seen.add(p.nhk)
            assert p.ipt * (h + 2) * ((1 << p.tw_log2) + 2) <= 320 or p.ipt == 1
    assert seen == {3, 4, 5}


def test_template_plan_tile_widths():
    for w, tw in ((1, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (100, 32)):
        p = R.template_plan(10, w, 64, "bf16")
        assert (1 << p.tw_log2, p.TH, p.halo_pix, p.nchunks) == (tw, 256 // tw, (tw + 2) * (256 // tw + 2), 2)
    assert R.template_plan(10, 20, 64, "fp32").nchunks == 4


def test_dispatch_rule_restatement():
    for cus in (256, 304, 8):
        (a, b, c) = R.rule_probes(cus)
        assert not R.small_preferred(*a, cus) and R.small_preferred(*b, cus) and R.small_preferred(*c, cus)
        assert R.small_preferred(*a, cus, opt3=2) and not R.small_preferred(*b, cus, opt3=0)
        assert a[0] * 4 >= 3 * cus > b[0] * 4
    # 256 -> 256 @16x16 on 256 CUs (csrc/conv3x3_small.hip): B = 32 runs on the small kernel, B = 64 on the template
    assert R.small_preferred(32, 16, 16, 256, 256, 256) and not R.small_preferred(64, 16, 16, 256, 256, 256)
