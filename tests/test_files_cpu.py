"""CPU: wu.files, the reader behind the metric and baseline commands, as far as it runs without a GPU: the two listing rules, the size
groups of a paired pass, the host half of the padded batch, the decoder context without a switch and the mixed-size error."""
import os
import subprocess
import sys

import numpy as np
import pytest

NAMES = ("a.jpg", "b.png", "c.jpeg", "d.JPG", "B.PNG", "e.txt")


def test_the_two_listing_rules(tmp_path):
    """image_files: *.jpg + *.png, case-sensitive, Path objects, sorted (pytorch-fid's listing).  pair_files: .jpg / .jpeg / .png in either
    case, str paths, sorted by stem.  fid and paired hand out these very functions."""
    from wu import fid, files, paired
    for n in NAMES:
        (tmp_path / n).write_bytes(b"")
    listed = files.image_files(str(tmp_path))
    assert listed == [tmp_path / "a.jpg", tmp_path / "b.png"]
    assert files.image_files(tmp_path) == listed
    pairs = files.pair_files(str(tmp_path), str(tmp_path))
    assert all(isinstance(p, str) and p == q for p, q in pairs)
    assert [os.path.basename(p) for p, _ in pairs] == ["B.PNG", "a.jpg", "b.png", "c.jpeg", "d.JPG"]
    assert [os.path.splitext(os.path.basename(p))[0] for p, _ in pairs] == ["B", "a", "b", "c", "d"]
    assert fid.image_files is files.image_files and paired.pair_files is files.pair_files


def test_size_groups_of_a_paired_pass(tmp_path):
    """Three pairs of 8 x 6 and two of 5 x 7 (Pillow sizes, w x h) in slices of 2: the group (5, 7) first, one slice of 2; then (8, 6),
    2 + 1; inside a group the pairs keep their sorted order.  One unequal pair is a ValueError that names both files."""
    from PIL import Image
    from wu import files
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    sizes = {"p0": (8, 6), "p1": (5, 7), "p2": (8, 6), "p3": (5, 7), "p4": (8, 6)}
    for stem, (w, h) in sizes.items():
        for d in (a, b):
            Image.fromarray(np.zeros((h, w, 3), dtype=np.uint8), "RGB").save(str(d / (stem + ".png")))
    got = files.pair_slices(files.pair_files(str(a), str(b)), 2)
    stems = [(size, [os.path.basename(pa)[:2] for pa, _ in part]) for size, part in got]
    assert stems == [((5, 7), ["p1", "p3"]), ((8, 6), ["p0", "p2"]), ((8, 6), ["p4"])]
    assert all(os.path.basename(pa) == os.path.basename(pb) and pa != pb for _, part in got for pa, pb in part)
    Image.fromarray(np.zeros((6, 9, 3), dtype=np.uint8), "RGB").save(str(b / "p2.png"))
    with pytest.raises(ValueError) as e:
        files.pair_slices(files.pair_files(str(a), str(b)), 2)
    assert str(a / "p2.png") in str(e.value) and str(b / "p2.png") in str(e.value)
    assert "is 8 x 6 but" in str(e.value) and "is 9 x 6" in str(e.value)


def test_host_half_of_the_padded_batch():
    """Arrays of one size: np.stack of them.  Ragged: (N, Hmax, Wmax, 3), each image in its corner, zero elsewhere, sizes as ints."""
    from wu import files
    rng = np.random.default_rng(0)
    same = [rng.integers(1, 256, (4, 5, 3), dtype=np.uint8) for _ in range(3)]
    host, sizes = files.padded_host(same)
    assert host.dtype == np.uint8 and np.array_equal(host, np.stack(same)) and sizes == [(4, 5)] * 3
    shapes = [(4, 5), (2, 7), (6, 1)]
    ragged = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    host, sizes = files.padded_host(ragged)
    assert host.shape == (3, 6, 7, 3) and host.dtype == np.uint8
    assert sizes == shapes and all(type(v) is int for s in sizes for v in s)
    for k, (a, (h, w)) in enumerate(zip(ragged, shapes)):
        assert np.array_equal(host[k, :h, :w], a)
        outside = host[k].copy()
        outside[:h, :w] = 0
        assert not outside.any()


def test_decoder_context_without_a_switch_imports_no_decoder():
    """In a fresh interpreter: importing wu.files and entering the context with every switch off yields None and has loaded neither
    decoder module nor the kernel library's binding."""
    import wu
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "from wu import files\n"
            "with files.pass_decoder() as dec:\n"
            "    assert dec is None\n"
            "with files.pass_decoder(False, False, False) as dec:\n"
            "    assert dec is None\n"
            "loaded = [m for m in ('wu.jpeg', 'wu.png', 'wu._lib', 'wu.resample', 'wu.input_pipeline') if m in sys.modules]\n"
            "assert not loaded, loaded\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.dirname(os.path.dirname(os.path.abspath(wu.__file__)))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_same_size():
    from wu import files
    files.same_size([(4, 5)] * 3, "in somewhere: ")
    files.same_size([(np.int64(4), np.int32(5)), (4, 5)], "in somewhere: ")
    with pytest.raises(ValueError) as e:
        files.same_size([(6, 1), (4, 5), (6, 1), (2, 7)], "in somewhere: ")
    assert str(e.value) == "images of different sizes in somewhere: [(2, 7), (4, 5), (6, 1)]"
    with pytest.raises(ValueError, match="--size"):
        files.same_size([(6, 1), (4, 5)], "(", "): give --size")
