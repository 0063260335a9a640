"""CPU oracle of wu.grid: torchvision 0.3's ``make_grid`` restated in torch ops (torchvision is not a dependency of this project), the
two pictures the reference builds with it, and an interpreter of a planned cell list.  Test infrastructure only.

``norm_ip``'s arithmetic is the project's settled restatement (wu.infer_driver.normalize_minmax): clamp to [lo, hi], subtract lo, divide
by ``hi - lo + 1e-5`` with every operation in fp32 -- ``lo`` / ``hi`` are kept as 0-dim fp32 tensors, so the denominator is two fp32
operations, not Python double arithmetic.  Everything works on whatever device its inputs are on (the benchmark gives it CUDA tensors
as the torch-op baseline).
"""
import math

import torch


def norm_ip(img, lo, hi):
    """torchvision/utils.py (0.3) make_grid.norm_ip: ``img.clamp_(min=min, max=max); img.add_(-min).div_(max - min + 1e-5)``, in place."""
    lo = torch.as_tensor(lo, dtype=torch.float32, device=img.device)
    hi = torch.as_tensor(hi, dtype=torch.float32, device=img.device)
    img.clamp_(min=lo, max=hi)
    img.sub_(lo).div_(hi - lo + 1e-5)


def norm_range(t, value_range):
    if value_range is not None:
        norm_ip(t, value_range[0], value_range[1])
    else:
        norm_ip(t, t.min(), t.max())


def make_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0):
    """torchvision 0.3 ``make_grid`` for three-channel input, line by line: stack a list, lift (3, H, W) to a batch, clone and normalise
    (per image with ``scale_each``, else the whole tensor), the ``size(0) == 1`` early return, then ``new_full`` and one
    ``narrow(...).copy_`` per image."""
    if isinstance(tensor, (list, tuple)):
        tensor = torch.stack(list(tensor), dim=0)
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    assert tensor.dim() == 4 and tensor.size(1) == 3
    tensor = tensor.float()
    if normalize is True:
        tensor = tensor.clone()
        if value_range is not None:
            assert isinstance(value_range, tuple)
        if scale_each is True:
            for t in tensor:
                norm_range(t, value_range)
        else:
            norm_range(tensor, value_range)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid


def to_u8(grid):
    """save_image's bytes (torchvision 0.3): ``grid.mul(255).clamp(0, 255).byte()``, channels last -- (..., 3, H, W) -> (..., H, W, 3)."""
    return grid.mul(255).clamp(0, 255).to(torch.uint8).movedim(-3, -1).contiguous()


def demo_tables(batch, results):
    """demo.py:74-82 for every angle: ``feats = [make_grid(batch, nrow=1, normalize=True, scale_each=True)]``, per axis
    ``res = (res + 1.) * 127.5; feats.append(make_grid(res, nrow=1, normalize=True, scale_each=True))``, ``torch.cat(feats, 2)``.
    ``results``: (T, nc, B, 3, H, W).  Returns (T, 3, Hg, Wg) fp32."""
    tables = []
    for t in range(results.shape[0]):
        feats = [make_grid(batch, nrow=1, normalize=True, scale_each=True)]
        for a in range(results.shape[1]):
            res = (results[t, a].float() + 1.) * 127.5
            feats.append(make_grid(res, nrow=1, normalize=True, scale_each=True))
        tables.append(torch.cat(feats, 2))
    return torch.stack(tables)


def summary_image(images, ref_images, fakes):
    """t_cls_train.py:324,361-363,375-377: ``blank = zeros_like(images[0]).unsqueeze(0)``; ``ref_img = cat([blank] + split(ref_images, 1),
    dim=3)``; ``in_out_img = cat([images] + fake_out_li, dim=3)``; ``res_img = cat([ref_img, in_out_img], dim=0)``;
    ``make_grid(res_img, nrow=1, normalize=True, scale_each=True)``.  ``fakes[i]`` is ``fake_out_li[i]``."""
    images, ref_images, fakes = images.float(), ref_images.float(), fakes.float()
    blank = torch.zeros_like(images[0]).unsqueeze(0)
    ref_img = torch.cat([blank] + list(torch.split(ref_images, 1)), dim=3)
    in_out_img = torch.cat([images] + [fakes[i] for i in range(fakes.shape[0])], dim=3)
    res_img = torch.cat([ref_img, in_out_img], dim=0)
    return make_grid(res_img, nrow=1, normalize=True, scale_each=True)


def emulate(plan, sources, pad_value=0.0, out="float"):
    """Interpreter of a wu.grid plan in torch ops -- what wu_grid_compose computes (include/wu_kernels.h), cell by cell: the group
    ranges over the pre-transformed fp32 values of all cells of a group (blank cells count with zeros), then clamp / subtract / divide
    and the copy into the frame.  Returns ((F, 3, Hg, Wg) fp32 or (F, Hg, Wg, 3) uint8, ranges (n_groups, 2))."""
    if not isinstance(sources, dict):
        sources = {"x": sources}
    f, hg, wg = plan.shape
    vals = []
    for c in plan.cells:
        if c.source is None:
            v = torch.zeros(3, c.h, c.w)
        else:
            s = sources[c.source]
            v = (s[c.index[0]] if isinstance(s, (list, tuple)) else s[c.index]).detach().cpu().float()
            assert tuple(v.shape) == (3, c.h, c.w)
            if c.pre:
                v = (v + 1.) * 127.5
        vals.append(v)
    ranges = torch.zeros(plan.n_groups, 2)
    for g in range(plan.n_groups):
        mine = [v for c, v in zip(plan.cells, vals) if c.group == g and c.normalize and c.value_range is None]
        if mine:
            ranges[g, 0] = min(v.min() for v in mine)
            ranges[g, 1] = max(v.max() for v in mine)
    grid = torch.full((f, 3, hg, wg), float(pad_value))
    for c, v in zip(plan.cells, vals):
        assert 0 <= c.frame < f and c.y0 >= 0 and c.x0 >= 0 and c.y0 + c.h <= hg and c.x0 + c.w <= wg
        if c.normalize:
            v = v.clone()
            lo, hi = c.value_range if c.value_range is not None else (ranges[c.group, 0], ranges[c.group, 1])
            norm_ip(v, lo, hi)
        grid[c.frame, :, c.y0:c.y0 + c.h, c.x0:c.x0 + c.w] = v
    return (to_u8(grid) if out == "uint8" else grid), ranges
