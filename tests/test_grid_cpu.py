"""CPU: the planners of wu.grid against the literal restatement of torchvision 0.3's make_grid (tests/_grid_ref.py), the geometry of
every plan, and the host-side validation of wu_grid_compose.  No GPU, no launch."""
import itertools

import pytest
import torch

import _grid_ref as R


def _imgs(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g) * 1.5


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("nrow", [1, 2, 8])
@pytest.mark.parametrize("padding", [0, 2])
def test_plan_grid_equals_make_grid(n, nrow, padding):
    from wu import grid
    x = _imgs(n, 5, 7, seed=n)
    for normalize, scale_each, vr, pad_value in itertools.product([False, True], [False, True], [None, (-1.0, 1.0)], [0.0, 0.5]):
        plan = grid.plan_grid(n, 5, 7, nrow, padding, normalize, vr, scale_each)
        got, _ = R.emulate(plan, x, pad_value)
        want = R.make_grid(x, nrow, padding, normalize, vr, scale_each, pad_value)
        assert got.shape[0] == 1 and torch.equal(got[0], want), (n, nrow, padding, normalize, scale_each, vr, pad_value)
        got8, _ = R.emulate(plan, x, pad_value, out="uint8")
        assert torch.equal(got8[0], R.to_u8(want))


def test_known_shapes():
    from wu import grid
    assert grid.plan_demo_tables(2, 3, 2, 8, 8).shape == (2, 22, 48)
    assert grid.plan_summary(2, 8, 8).shape == (1, 32, 28)
    plan = grid.plan_grid(3, 5, 7, nrow=2)
    assert plan.shape == (1, 16, 20) and len(plan.cells) == 3
    got, _ = R.emulate(plan, _imgs(3, 5, 7), pad_value=0.5)
    assert torch.all(got[0, :, 9:14, 11:18] == 0.5)                      # the empty cell of the ragged row
    assert grid.plan_grid(1, 5, 7).shape == (1, 5, 7)                     # one image: no border


def test_constant_image_normalises_to_zeros():
    from wu import grid
    x = torch.full((2, 3, 4, 4), 0.75)
    got, rng = R.emulate(grid.plan_grid(2, 4, 4, normalize=True, scale_each=True), x)
    assert torch.equal(got, R.make_grid(x, normalize=True, scale_each=True)[None])
    assert torch.all(got[0, :, 2:6, 2:6] == 0) and torch.equal(rng, torch.full((2, 2), 0.75))


def test_plan_demo_tables_equals_the_script():
    from wu import grid
    T, nc, B, h, w = 2, 3, 2, 8, 8
    batch, results = _imgs(B, h, w, 1), _imgs(T * nc * B, h, w, 2).view(T, nc, B, 3, h, w)
    plan = grid.plan_demo_tables(T, nc, B, h, w)
    got, _ = R.emulate(plan, {"batch": batch, "results": results})
    assert torch.equal(got, R.demo_tables(batch, results))
    # B == 1: make_grid returns the image alone
    got1, _ = R.emulate(grid.plan_demo_tables(T, nc, 1, h, w), {"batch": batch[:1], "results": results[:, :, :1]})
    assert torch.equal(got1, R.demo_tables(batch[:1], results[:, :, :1]))


def test_plan_summary_equals_the_training_script():
    from wu import grid
    B, h, w = 2, 8, 8
    images, ref, fakes = _imgs(B, h, w, 3), _imgs(B, h, w, 4).abs() + 0.5, _imgs(B * B, h, w, 5).view(B, B, 3, h, w)
    plan = grid.plan_summary(B, h, w)
    got, rng = R.emulate(plan, {"images": images, "ref": ref, "fakes": fakes})
    assert torch.equal(got[0], R.summary_image(images, ref, fakes))
    assert rng[0, 0] == 0 and rng[0, 1] == ref.max()                      # ref > 0 everywhere: strip 0's minimum is the blank's zero
    assert ref.min() > 0


def _plans():
    from wu import grid
    for n, nrow, padding in itertools.product([1, 2, 3, 5, 9], [1, 2, 8], [0, 2, 3]):
        yield grid.plan_grid(n, 5, 7, nrow, padding, True, None, True)
    yield grid.plan_demo_tables(2, 3, 2, 8, 8)
    yield grid.plan_demo_tables(3, 5, 1, 6, 4)
    yield grid.plan_summary(2, 8, 8)
    yield grid.plan_summary(1, 3, 5)


def test_cells_do_not_overlap_and_stay_inside_their_frame():
    n_plans = 0
    for plan in _plans():
        f, hg, wg = plan.shape
        cover = torch.zeros(f, hg, wg, dtype=torch.int32)
        for c in plan.cells:
            assert 0 <= c.frame < f and c.h > 0 and c.w > 0
            assert 0 <= c.y0 and c.y0 + c.h <= hg and 0 <= c.x0 and c.x0 + c.w <= wg
            assert 0 <= c.group < plan.n_groups
            cover[c.frame, c.y0:c.y0 + c.h, c.x0:c.x0 + c.w] += 1
        assert int(cover.max()) == 1
        n_plans += 1
    assert n_plans > 45


def test_abi_validation_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    assert lib.wu_grid_cell_bytes() == 72
    assert lib.wu_grid_workspace_bytes(0, 1) == 0 and lib.wu_grid_workspace_bytes(1, 0) == 0
    ws = lib.wu_grid_workspace_bytes(4, 3)
    assert ws >= 2 * 3 * 8
    import ctypes
    off = (ctypes.c_longlong * 2)()
    assert lib.wu_grid_workspace_layout(4, 3, off) == 0 and 0 <= off[0] and off[0] + 3 * 8 <= ws and off[0] % 8 == 0
    assert lib.wu_grid_workspace_layout(4, -1, off) < 0 and b"counts" in lib.wu_last_error()
    F, Hg, Wg = 2, 10, 12
    fake = 1 << 20                                                     # never dereferenced: every case below is refused before a launch
    def call(n_cells=4, n_groups=3, ws_bytes=ws, out_bytes=F * Hg * Wg * 3, kind=1, frames=F, hg=Hg, wg=Wg, cells=fake, wsp=fake, out=fake):
        return lib.wu_grid_compose(cells, n_cells, n_groups, wsp, ws_bytes, out, out_bytes, kind, frames, hg, wg, 0.0, None)
    for kw, word in (({"n_cells": 0}, b"counts"), ({"n_groups": 0}, b"counts"), ({"n_cells": -3}, b"counts"),
                     ({"frames": 0}, b"geometry"), ({"hg": 0}, b"geometry"), ({"wg": -1}, b"geometry"),
                     ({"kind": 2}, b"out_kind"), ({"kind": -1}, b"out_kind"),
                     ({"out_bytes": F * Hg * Wg * 3 - 1}, b"output too small"),
                     ({"kind": 0, "out_bytes": F * Hg * Wg * 3 * 4 - 1}, b"output too small"),
                     ({"ws_bytes": ws - 1}, b"workspace too small"),
                     ({"cells": None}, b"null"), ({"wsp": None}, b"null"), ({"out": None}, b"null"),
                     ({"out": fake + 4}, b"aligned")):
        assert call(**kw) < 0, kw
        assert word in lib.wu_last_error(), (kw, lib.wu_last_error())


def test_python_layer_refuses_cpu_tensors_and_grey_input():
    from wu import grid, infer_driver
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no CPU"):
        grid.make_grid(x)
    with pytest.raises(RuntimeError, match="There is no CPU"):
        grid.demo_tables(x, torch.zeros(1, 2, 2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="There is no CPU"):
        grid.summary_image(x, x, torch.zeros(2, 2, 3, 4, 4))
    with pytest.raises(ValueError, match="grey"):
        grid.make_grid(torch.zeros(2, 1, 4, 4))
    with pytest.raises(TypeError):
        grid.make_grid(x, bogus=1)
    for name in ("save_grid", "demo_frames", "save_demo"):
        assert callable(getattr(infer_driver, name))


def test_plan_grid_checks_its_arguments_in_front_of_the_cache():
    from wu import grid
    with pytest.raises(ValueError, match="value_range"):
        grid.plan_grid(2, 4, 4, normalize=True, value_range=[-1.0, 1.0])       # a list: unhashable, and not a tuple
    with pytest.raises(ValueError, match="bad geometry"):
        grid.plan_grid(0, 4, 4)
    assert grid.plan_grid(2, 4, 4, normalize=1, value_range=(-1, 1)) is grid.plan_grid(2, 4, 4, normalize=True, value_range=(-1.0, 1.0))


def test_descriptors_are_worked_out_from_the_base_tensor():
    """GridComposer._describe computes every cell's pointer and strides from its source tensor; it must equal taking the view."""
    import torch
    from wu import grid
    comp = object.__new__(grid.GridComposer)
    comp._templates, comp.device, comp.MAX_CACHED = {}, torch.device("cpu"), 64
    T, nc, B, h, w = 2, 3, 2, 5, 7
    batch = torch.zeros(B, 3, h + 2, w + 3)[:, :, 1:h + 1, 2:w + 2]
    results = torch.zeros(T, nc, B, 3, h, w, dtype=torch.bfloat16).permute(0, 1, 2, 3, 5, 4).contiguous().permute(0, 1, 2, 3, 5, 4)
    plan = grid.plan_demo_tables(T, nc, B, h, w)
    src = {"batch": batch, "results": results}
    d = comp._describe(plan, src)
    for i, c in enumerate(plan.cells):
        t = src[c.source][c.index]
        assert d["src"][i] == t.data_ptr() and (d["sc"][i], d["sy"][i], d["sx"][i]) == t.stride()
        assert bool(d["flags"][i] & grid.F_BF16) == (t.dtype == torch.bfloat16) and bool(d["flags"][i] & grid.F_PRE) == c.pre
        assert (d["h"][i], d["w"][i], d["frame"][i], d["y0"][i], d["x0"][i], d["group"][i]) == (c.h, c.w, c.frame, c.y0, c.x0, c.group)
    lst = [torch.zeros(3, h, w) for _ in range(3)]
    d = comp._describe(grid.plan_grid(3, h, w, nrow=2), {"x": lst})
    assert [int(p) for p in d["src"]] == [t.data_ptr() for t in lst]
    blank = comp._describe(grid.plan_summary(2, h, w), {"images": batch, "ref": batch, "fakes": torch.zeros(2, 2, 3, h, w)})
    assert blank["src"][0] == 0 and blank["flags"][0] & grid.F_BLANK
    with pytest.raises(IndexError):
        comp._describe(grid.plan_grid(3, h, w), {"x": batch})
