"""The oracle of tests/test_gpu_pointwise_exact.py, checked without a GPU for EVERY case that file runs: the worst-case sum stays below
2^24, the fp32 reference equals the float64 reference exactly, the premises that make a wrong kernel visible hold on the reference (values
bf16 cannot hold, exact zeros in front of the activation, exact zeros in the gate), the stride-2 row maps are autograd's, and the tables
cover what they were written to cover (K-step counts, tile heights, parities of the strided sizes) -- asserted from the tables."""
import pytest
import torch
import torch.nn.functional as F

import _pointwise_ref as R

MIN_UNREPRESENTABLE = 0.01


def _integers_below_2_24(v64, bound):
    assert v64.dtype == torch.float64
    assert bool((v64 == v64.round()).all()) and float(v64.abs().max()) <= bound < R.TWO24


def _premises(lin, out, gate, bf16, what):
    assert int((lin == 0).sum()) > 0, f"{what}: no exact zero in front of the activation"
    if gate is not None:
        assert int((gate == 0).sum()) > 0, f"{what}: no exact zero in the gate"
    if bf16:
        frac = R.unrepresentable(out)
        assert frac >= MIN_UNREPRESENTABLE, f"{what}: only {frac:.4f} of the values in front of the rounding are not bf16 values"


@pytest.mark.parametrize("c", R.PW_CASES, ids=lambda c: c.name)
def test_pointwise_cases(c):
    assert R.pw_bound(c) < R.TWO24
    ops = R.pw_operands(c)
    for t in (ops["x"], ops["w"], ops["res"], ops["gate"]):
        assert t is None or float(t.abs().max()) <= 256          # exact in bf16
    lin, out = R.pw_reference(c, ops)
    lin64, out64 = R.pw_reference(c, ops, torch.float64)
    assert float(lin.abs().max()) <= R.pw_bound(c)
    assert torch.equal(lin, lin64) and torch.equal(out, out64)
    assert out.shape == (c.n, c.cout, c.hout, c.wout)
    _premises(lin, out, ops["gate"], c.dtype == "bf16", c.name)
    has_b, has_r, _, gact = R.EPILOGUES[c.epi]
    assert (ops["bias"] is not None) == has_b and (ops["res"] is not None) == has_r and (ops["gate"] is not None) == (gact != R.NONE)


def test_pointwise_linear_part_is_an_integer_in_float64():
    for c in R.PW_CASES[::7]:
        ops = R.pw_operands(c)
        x, w = ops["x"].double(), ops["w"].double()
        xs = R.gather_rows(x) if c.in_stride == 2 else x
        worst = torch.einsum("oc,nchw->nohw", w.abs(), xs.abs())
        _integers_below_2_24(worst + (ops["bias"].abs().max().double() if ops["bias"] is not None else 0) + R.RR, R.pw_bound(c))


@pytest.mark.parametrize("hw", [(9, 7), (8, 6), (10, 8), (10, 7), (1, 1), (2, 2)])
def test_stride2_row_maps_are_autograd_of_a_strided_conv(hw):
    """The gather equals a stride-2 1x1 F.conv2d; the scatter equals its gradient with respect to the input (on real operands, fp64)."""
    h, w = hw
    g = torch.Generator().manual_seed(7)
    x = torch.rand((2, 5, h, w), generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.rand((3, 5), generator=g, dtype=torch.float64)
    y = F.conv2d(x, wt.view(3, 5, 1, 1), stride=2)
    assert torch.equal(y, F.conv2d(R.gather_rows(x), wt.view(3, 5, 1, 1)))
    assert y.shape[2:] == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    dy = torch.rand(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    # the data gradient: the GEMM w^T . dy on the coarse grid, scattered
    want = R.scatter_rows(F.conv2d(dy, wt.t().reshape(5, 3, 1, 1)), h, w)
    assert (x.grad - want).abs().max().item() <= 1e-12
    own = torch.zeros((h, w), dtype=torch.bool)
    own[::2, ::2] = True
    assert bool((want[:, :, ~own] == 0).all())


def test_pointwise_table_covers_what_it_was_written_for():
    s1 = [c for c in R.PW_CASES if c.in_stride == 1 and c.out_stride == 1]
    for dtype in ("bf16", "fp32"):
        for tile in (64, 128, 256):
            mine = [c for c in s1 if c.dtype == dtype and c.tile == tile]
            assert {c.cin // R.K_PER_STEP[dtype] for c in mine} >= {1, 2, 3, 4, 5, 6}, (dtype, tile)
            assert {c.epi for c in mine} >= set(R.EPI_ORDER), (dtype, tile)
            ragged = [c for c in mine if c.wc % tile != 0 and c.wc > tile]
            assert ragged, (dtype, tile)
        assert {c.cout for c in s1 if c.dtype == dtype} >= {64, 192}
        assert any(c.n * c.hc * c.wc < 32 for c in s1 if c.dtype == dtype)
    assert all(c.cin % R.K_PER_STEP[c.dtype] == 0 and c.cout % 64 == 0 and c.tile in R.TILE_OPTION for c in R.PW_CASES)
    gathers = [c for c in R.PW_CASES if c.in_stride == 2]
    for dtype in ("bf16", "fp32"):
        assert {(c.hin % 2, c.win % 2) for c in gathers if c.dtype == dtype} >= {(1, 1), (0, 0)}
    scatters = [c for c in R.PW_CASES if c.out_stride == 2]
    for epi in ("bare", "res_gate"):
        forms = {(c.hout - 2 * c.hc, c.wout - 2 * c.wc) for c in scatters if c.epi == epi and c.dtype == "bf16"}
        assert forms >= {(0, 0), (-1, -1), (0, -1)}, (epi, forms)
    assert {c.dtype for c in scatters} == {"bf16", "fp32"}
    assert {c.tile for c in gathers + scatters} == {64, 128, 256}
    assert len({c.name for c in R.PW_CASES}) == len(R.PW_CASES) and len({c.seed for c in R.PW_CASES}) == len(R.PW_CASES)


def test_persistent_kernel_cases_are_walked_on_the_forced_grid():
    walked, small = R.pw3_cases()
    assert small and all(c.n * c.hc * c.wc < 32 for c in small)
    assert any(c.cout == 192 for c in walked) and any(c.cout % 128 == 0 for c in walked) and any(c.cout == 64 for c in walked)
    assert {c.epi for c in walked} >= set(R.EPI_ORDER)
    assert {c.cin // 64 for c in walked} >= {1, 2, 3, 4, 5, 6}
    grids = set()
    for opt in R.PW3_OPTIONS:
        for c in walked:
            items, grid = R.pw3_plan(c.wc, c.cout, opt, R.PW3_FORCED_CUS)
            assert items // grid >= 2, (c.name, opt, items, grid)
            grids.add(grid)
    assert grids == {3, 6}
    assert all(c.wc % 128 != 0 for c in walked)          # a ragged last tile


@pytest.mark.parametrize("c", R.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_cases(c):
    b1, b2 = R.chain_bounds(c)
    assert b1 < R.TWO24 and b2 < R.TWO24
    ops = R.chain_operands(c)
    for k in ("x", "wa", "wb", "res", "gate1", "gate2"):
        assert ops[k] is None or float(ops[k].abs().max()) <= 256
    lin1, y1, lin2, y2 = R.chain_reference(c, ops)
    ref64 = R.chain_reference(c, ops, torch.float64)
    for a, b in zip((lin1, y1, lin2, y2), ref64):
        assert torch.equal(a, b)
    assert float(lin1.abs().max()) <= b1 and float(lin2.abs().max()) <= b2
    y1r = y1.bfloat16().float()
    assert bool((y1r == y1r.round()).all()) and float(y1r.abs().max()) <= b1 + b1 // 256 + 1       # a rounded integer is an integer
    _premises(lin1, y1, ops["gate1"], True, c.name + " stage 1")
    _premises(lin2, y2, ops["gate2"], True, c.name + " stage 2")
    assert not torch.equal(y1r, y1), "the rounding of y1 does not show in the second GEMM's operand"


def test_chain_table_covers_what_it_was_written_for():
    for form in ("forward", "backward"):
        mine = [c for c in R.CHAIN_CASES if c.form == form]
        assert {c.k1 for c in mine} == {64, 128, 256} and {c.c1 for c in mine} == {256, 512, 1024}
        assert {c.c2 for c in mine} == {32, 64, 160} and {c.m for c in mine} == {5, 37, 70}
        assert all(c.c2 > R.CHAIN_ZERO_ROW for c in mine)


@pytest.mark.parametrize("c", R.S2_CASES, ids=lambda c: c.name)
def test_stride2_conv_cases(c):
    bf, bd = R.s2_bounds(c)
    assert bf < R.TWO24 and bd < R.TWO24
    ops = R.s2_operands(c)
    for k in ("x", "w", "gate", "dy", "xgate"):
        assert float(ops[k].abs().max()) <= 256
    for epi in R.S2_FWD_EPILOGUES:
        lin, out = R.s2_forward_reference(c, ops, epi)
        lin64, out64 = R.s2_forward_reference(c, ops, epi, torch.float64)
        assert torch.equal(lin, lin64) and torch.equal(out, out64) and float(lin.abs().max()) <= bf
        _premises(lin, out, ops["gate"] if R.S2_FWD_EPILOGUES[epi][1] != R.NONE else None, True, f"{c.name} forward {epi}")
    for epi in R.S2_DGRAD_EPILOGUES:
        lin, out = R.s2_dgrad_reference(c, ops, epi)
        lin64, out64 = R.s2_dgrad_reference(c, ops, epi, torch.float64)
        assert torch.equal(lin, lin64) and torch.equal(out, out64) and float(lin.abs().max()) <= bd
        assert out.shape == (c.n, c.cin, c.h, c.w)
        _premises(lin, out, ops["xgate"] if R.S2_DGRAD_EPILOGUES[epi] != R.NONE else None, True, f"{c.name} data gradient {epi}")
    # the data gradient is autograd's
    x = torch.zeros((c.n, c.cin, c.h, c.w), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, ops["w"].double(), stride=2, padding=1).backward(ops["dy"].double())
    assert torch.equal(x.grad.float(), R.s2_dgrad_reference(c, ops, "ungated")[0])


def test_stride2_conv_table_covers_what_it_was_written_for():
    assert {(c.h, c.w) for c in R.S2_CASES} >= {(2, 2), (5, 7), (11, 13), (12, 10), (9, 8)}
    assert {c.cin for c in R.S2_CASES} == {64, 128} and {c.cout for c in R.S2_CASES} == {64, 128, 192}
    assert any(c.cout == 192 and (c.h, c.w) == (9, 8) for c in R.S2_CASES) and max(c.n for c in R.S2_CASES) == 3
    walked = [c for c in R.S2_CASES if c.walked]
    assert walked
    for c in walked:
        rows = c.n * ((c.h - 1) // 2 + 1) * ((c.w - 1) // 2 + 1)
        for items, grid in (R.pw3_conv_plan(rows, c.cout, 1, R.S2_FORCED_CUS), R.pw3_conv_plan(rows, c.cin, 4, R.S2_FORCED_CUS)):
            assert grid == 2 * R.S2_FORCED_CUS and items // grid >= 2
    # a 128-row tile spans an image border: more than one image in fewer rows than a tile
    assert any(c.n > 1 and ((c.h - 1) // 2 + 1) * ((c.w - 1) // 2 + 1) < 128 for c in R.S2_CASES)


@pytest.mark.parametrize("c", R.STEM_FWD_CASES, ids=lambda c: c.name)
def test_stem_forward_cases(c):
    bound = R.stem_bounds()[0]
    assert bound < R.TWO24
    ops = R.stem_operands(c)
    assert float(ops["x"].abs().max()) <= 256 and float(ops["w"].abs().max()) <= 256        # the matrix-core kernel rounds both to bf16
    lin, out = R.stem_forward_reference(c, ops)
    lin64, out64 = R.stem_forward_reference(c, ops, torch.float64)
    assert torch.equal(lin, lin64) and torch.equal(out, out64) and float(lin.abs().max()) <= bound
    assert out.shape == (c.n, 64) + R.stem_out(c.h, c.w)
    _premises(lin, out, None, True, c.name)


@pytest.mark.parametrize("c", R.STEM_DGRAD_CASES, ids=lambda c: c.name)
def test_stem_dgrad_cases(c):
    bound = R.stem_bounds()[1]
    assert bound < R.TWO24
    ops = R.stem_dgrad_operands(c)
    assert float(ops["dy"].abs().max()) <= 256 and float(ops["w"].abs().max()) <= 256
    dx = R.stem_dgrad_reference(c, ops)
    assert torch.equal(dx, R.stem_dgrad_reference(c, ops, torch.float64))
    assert float((dx + ops["dx0"]).abs().max()) <= bound and float(dx.abs().max()) > 0
    even = c.h % 2 == 0 and c.w % 2 == 0
    assert {"mfma": even, "valu_bf16": not even, "fp32": True}[c.kind]


def test_stem_tables_cover_what_they_were_written_for():
    assert {(c.h, c.w) for c in R.STEM_FWD_CASES} == {(7, 7), (20, 36), (33, 70), (16, 130)}
    assert {(c.h, c.w, c.act) for c in R.STEM_FWD_CASES} == {(h, w, a) for (h, w) in ((7, 7), (20, 36), (33, 70), (16, 130)) for a in (R.RELU, R.NONE)}
    assert all(c.n in (2, 3) for c in R.STEM_FWD_CASES)
    for c in R.STEM_FWD_CASES:           # two workgroups (one CU): at least three tiles each on the multi-tile images
        if (c.h, c.w) != (7, 7):
            assert R.stem_fwd_tiles(c) // 2 >= 3, c.name
    ho, wo = R.stem_out(33, 70)
    assert ho % R.STEM_TH != 0 and wo % R.STEM_TW != 0          # ragged in both tile directions
    assert {(c.kind, c.h, c.w) for c in R.STEM_DGRAD_CASES} >= {("mfma", 8, 8), ("mfma", 34, 66)}
    assert {c.kind for c in R.STEM_DGRAD_CASES} == {"mfma", "valu_bf16", "fp32"}
    big = [c for c in R.STEM_DGRAD_CASES if (c.kind, c.h, c.w, c.n) == ("mfma", 34, 66, 2)]
    assert big and R.stem_dgrad_tiles(big[0]) // 2 >= 3
