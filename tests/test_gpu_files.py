"""wu.files on the GPU: read_batches through Pillow and through the PNG decoder give the same padded batches as the files read one by one,
and wu.fid's legacy resize rule refuses mixed sizes PER BATCH on its three read paths -- a directory whose batches are each of one size
is read, the same directory cut into batches that mix sizes is not."""
import numpy as np
import pytest
import torch

import _resample_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _save(directory, shapes, seed):
    """PNGs 0.png, 1.png, ... of the (h, w) given; returns (paths, the arrays)."""
    from PIL import Image
    images = [C.picture(h, w, "mixed", seed + i) for i, (h, w) in enumerate(shapes)]
    paths = []
    for i, a in enumerate(images):
        paths.append(str(directory / f"{i}.png"))
        Image.fromarray(a, "RGB").save(paths[-1])
    return paths, images


def test_read_batches(tmp_path):
    """Five 12 x 10 files in batches of 2: 2, 2, 1, each the np.stack of its files; the PNG decoder gives the same tensors and sizes.  A
    batch of (12, 10), (7, 16), (12, 10): padded to (3, 12, 16, 3), every image in its corner, on both paths."""
    from wu import files, png
    one, two = tmp_path / "one", tmp_path / "ragged"
    one.mkdir(), two.mkdir()
    paths, images = _save(one, [(12, 10)] * 5, 40)
    assert all(np.array_equal(files.read_rgb(p), a) for p, a in zip(paths, images))
    got = list(files.read_batches(paths, 2, device=DEV))
    assert [tuple(b.shape) for b, _ in got] == [(2, 12, 10, 3), (2, 12, 10, 3), (1, 12, 10, 3)]
    for k, (b, sizes) in enumerate(got):
        assert b.dtype == torch.uint8 and b.is_cuda and sizes == [(12, 10)] * b.shape[0]
        assert np.array_equal(b.cpu().numpy(), np.stack([files.read_rgb(p) for p in paths[2 * k:2 * k + 2]]))
    ragged, pictures = _save(two, [(12, 10), (7, 16), (12, 10)], 50)
    (pad, pad_sizes), = list(files.read_batches(ragged, 3, device=DEV))
    assert tuple(pad.shape) == (3, 12, 16, 3) and pad_sizes == [(12, 10), (7, 16), (12, 10)]
    for k, a in enumerate(pictures):
        assert np.array_equal(pad[k, :a.shape[0], :a.shape[1]].cpu().numpy(), a)
    with files.pass_decoder(gpu_decode_png=True) as dec:
        assert isinstance(dec, png.GPUPngDecoder)
        through = list(files.read_batches(paths, 2, dec))
        (dpad, dpad_sizes), = list(files.read_batches(ragged, 3, dec))
    assert len(through) == 3
    for (b, sizes), (db, dsizes) in zip(got, through):
        assert torch.equal(b, db.to(DEV)) and sizes == dsizes
    assert dpad_sizes == pad_sizes and tuple(dpad.shape) == (3, 12, 16, 3)
    for k, a in enumerate(pictures):
        assert np.array_equal(dpad[k, :a.shape[0], :a.shape[1]].cpu().numpy(), a)


def test_legacy_rule_refuses_mixed_sizes_per_batch(tmp_path):
    """Files that sort as 24 x 20, 24 x 20, 32 x 16, 32 x 16.  In batches of 2 every batch has one size: the legacy rule reads the
    directory on the Pillow, JPEG-decoder and PNG-decoder paths, with the same feature rows, those of the model on the two batches built
    by hand.  In batches of 3 the first batch mixes sizes: ValueError on all three paths."""
    import _inception_ref as IR
    from wu import fid
    from wu.features import FeatureBank
    from wu.inception import InceptionV3
    paths, images = _save(tmp_path, [(24, 20), (24, 20), (32, 16), (32, 16)], 60)
    assert [p.name for p in fid.image_files(str(tmp_path))] == ["0.png", "1.png", "2.png", "3.png"]
    model = InceptionV3()
    model.load_state_dict(IR.make_params(True, seed=3))
    want = torch.cat([model(torch.from_numpy(np.stack(images[i:i + 2])).to(DEV))[0].reshape(2, 2048) for i in (0, 2)])
    assert torch.isfinite(want).all()
    ways = ({}, {"gpu_decode": True}, {"gpu_decode_png": True})
    for kw in ways:
        bank = FeatureBank()
        mu, sigma = fid.statistics_of_path(str(tmp_path), model, 2, features=bank, **kw)
        assert mu.shape == (2048,) and sigma.shape == (2048, 2048) and bank.n == 4 and bank.resize == "legacy"
        assert torch.equal(bank.features, want), kw
    for kw in ways:
        with pytest.raises(ValueError):
            fid.statistics_of_path(str(tmp_path), model, 3, **kw)
