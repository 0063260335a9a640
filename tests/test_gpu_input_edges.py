"""The input kernels (csrc/image.hip, behind wu.input_pipeline.GPUInputPipeline) against the Pillow chain (oracle/input_ref.py) at the edge
cases of tests/_image_edge_cases.py: 1-pixel sources and crop windows, S = 1, exact integer scales, a 128.9x down-scale sharing its ksize
with up-scales, crops flush with the last row / column, rotations by 0 / +-360 / 90 / 180 / 270 / +-10 / 45 in both orders, and the
colour jitter over a factor grid, every order and flat / saturated / tie-mean images.  The padding of every source buffer is poisoned
(255, noise): a tap that strays out of its image shows.
Bar: BIT-EXACT, no tolerance anywhere.  Pillow is the reference; tests/test_input_edges_cpu.py holds the numpy restatement of the same
arithmetic to Pillow on the same cases, and shows that the jitter cases tell a fused blend (one rounding) from Pillow's (two).

Measured on an MI355X with image.hip built WITH contraction (v_fma_f32 in the blend): every geometry, crop and rotation case passed; of
jit_single_S64's 30 images the ten Contrast / Color ones at 2/3, 0.8, 1.1, 1.2, 4/3 failed with 212, 20, 107, 373, 845 / 129, 51, 107,
221, 570 of 12,288 values off by one byte -- exactly the counts the one-rounding emulation of the CPU test predicts -- and every
Brightness image passed."""
import numpy as np
import pytest
import torch

import _image_edge_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pipe(case):
    from wu.input_pipeline import GPUInputPipeline
    return GPUInputPipeline(case.S, augmentation=case.augmentation, train=case.train)


def _run(case, fill, params=None, pipe=None):
    src = torch.from_numpy(EC.padded(case, fill)).to(DEV)
    out = (pipe or _pipe(case))(src, case.sizes, params or case.params)
    assert tuple(out.shape) == (len(case.sizes), 3, case.S, case.S) and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("name", EC.ALL_CASES)
def test_edge_case_equals_pillow(name):
    """Every case, twice: padding 255 and padding noise.  Both equal Pillow, hence each other."""
    case = EC.CASES[name]
    want = EC.pillow(name)
    for fill in ("255", "noise"):
        got = _run(case, fill)
        assert np.array_equal(got, want), f"padding {fill}:\n" + EC.first_difference(case, got, want)


def test_workspace_reuse_across_scale_ranges():
    """One pipeline object: the up-scaling batch (ksize 3), the batch with the 128.9x down-scale (ksize 261), the up-scaling batch
    again on the grown workspace.  The workspace grows once; all three equal Pillow and the first equals the third bit for bit."""
    small, big = EC.CASES["geo_upscale_S8_test"], EC.CASES["geo_mixed_S8_test"]
    pipe = _pipe(small)
    first = _run(small, "noise", pipe=pipe)
    ws1 = pipe._ws
    second = _run(big, "noise", pipe=pipe)
    ws2 = pipe._ws
    third = _run(small, "noise", pipe=pipe)
    assert ws2 is not ws1 and ws2.numel() > ws1.numel() and pipe._ws is ws2
    for case, got in ((small, first), (big, second), (small, third)):
        assert np.array_equal(got, EC.pillow(case.name)), EC.first_difference(case, got, EC.pillow(case.name))
    assert np.array_equal(first, third)


@pytest.mark.parametrize("name", ["geo_mixed_S8_train", "geo_S33_train_flipped", "crop_windows_flipped", "rot_before_corner", "rot_after_S33"])
def test_staging_path_equals_direct_path(name):
    """Identity jitter -- order (0, 1, 2), factors (1, 1, 1) -- sends the geometry through the u8 staging buffer and the jitter kernel's
    epilogue; no jitter writes NCHW directly.  Same bytes either way, and Pillow's."""
    case = EC.CASES[name]
    direct = _run(case, "noise", [{**p, **EC.NO_JITTER} for p in case.params])
    staged = _run(case, "noise", [{**p, **EC.IDENTITY_JITTER} for p in case.params])
    assert np.array_equal(staged, direct), EC.first_difference(case, staged, direct)
    assert np.array_equal(direct, EC.pillow(name)), EC.first_difference(case, direct, EC.pillow(name))
