"""CPU: the LPIPS restatement (tests/_lpips_ref.py) against an independent torch float64 composition, its invariants, the state-dict
handling of wu.lpips and the size rule.  No kernel is launched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lpips_cases as CASES
import _lpips_ref as R


def _torch_head(fa, fb, w):
    """The lpips package's composition in float64: normalize_tensor, squared difference, the lin layer as a 1 x 1 conv2d, spatial mean."""
    fa, fb = torch.from_numpy(fa).double(), torch.from_numpy(fb).double()

    def norm(t):
        return t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + 1e-10)

    d = (norm(fa) - norm(fb)) ** 2
    return F.conv2d(d, torch.from_numpy(w).double().view(1, -1, 1, 1)).mean(dim=(2, 3))[:, 0].numpy()


@pytest.mark.parametrize("c", CASES.HEAD_CHANNELS)
def test_head_against_torch_composition(c):
    for h, w in CASES.head_pixel_maps(16):
        x, y = CASES.feature_maps(c, h, w, 3, CASES.HEAD_B, seed=c + h)
        lw = CASES.lin_weight(c, c)
        got = R.head(x[None], y, lw)
        assert got.shape == (3, CASES.HEAD_B) and got.dtype == np.float64 and np.isfinite(got).all()
        for r in range(3):
            want = _torch_head(x, y[r], lw)
            scale = np.abs(_torch_head(x, y[r], np.abs(lw))).max() + 1e-300
            assert np.abs(got[r] - want).max() <= 1e-12 * scale, (c, h, w, r)
        assert np.all(got[0] == 0.0)                                          # row 0 of y is x
        assert np.all(np.abs(got - R.head(x[None], y, lw)) == 0)
        assert np.all(R.head_bound(x[None], y, lw) >= 0)


def test_symmetry_identity_and_zero_vectors():
    x, y = CASES.feature_maps(64, 3, 5, 2, 2, seed=3)
    lw = CASES.lin_weight(64, 1)
    assert np.array_equal(R.head(x[None], y, lw), R.head(y, x[None], lw))
    assert np.all(R.head(y, y, lw) == 0.0)
    z = np.zeros_like(x)
    assert np.all(R.head(z, z, lw) == 0.0)
    one = R.head(z[None], y, np.abs(lw))                                      # zero vector against unit vectors: the weighted mean of yh^2
    assert np.isfinite(one).all() and np.all(one > 0)
    f = [np.stack([x, y[1], y[0]])] * 5                                       # (R = 3, B, C, h, w) for every "layer"
    lin = {f"lin{k}.model.1.weight": torch.from_numpy(np.abs(lw)).view(1, -1, 1, 1) for k in range(5)}
    pw = R.total(R.pairwise_layers(f, lin))
    assert pw.shape == (3, 3, 2) and np.array_equal(pw, pw.transpose(1, 0, 2)) and np.all(pw[[0, 1, 2], [0, 1, 2]] == 0.0)
    assert np.allclose(R.diversity(pw), (pw[0, 1] + pw[0, 2] + pw[1, 2]) / 3, rtol=1e-15)


def test_input_mapping_rounds_every_operation():
    v = np.random.default_rng(0).integers(0, 256, size=(2, 3, 5, 7)).astype(np.uint8)
    u = R.scale_input(v, "uint8")
    assert u.dtype == np.float32
    t = v.astype(np.float32) * np.float32(2.0 / 255.0)
    t = t + np.float32(-1.0)
    for c in range(3):
        want = (t[:, c] - np.float32(R.SHIFT[c])) / np.float32(R.SCALE[c])
        assert want.dtype == np.float32 and np.array_equal(u[:, c], want)
    f = (v.astype(np.float32) * np.float32(2.0 / 255.0) + np.float32(-1.0)).astype(np.float32)
    assert np.array_equal(R.scale_input(f, (-1, 1)), u)                       # the float path on v * 2 / 255 - 1
    nhwc = R.network_input(v, "uint8", bf16=True)
    assert nhwc.shape == (2, 5, 7, 16) and nhwc.dtype == torch.bfloat16 and torch.all(nhwc[..., 3:] == 0)


def test_size_rule():
    from wu import lpips
    alex, _ = R.make_params(CASES.PARAM_SEED)
    for fn in (lpips.feature_sizes, R.feature_sizes):
        with pytest.raises(ValueError, match="31"):
            fn(30, 31)
        with pytest.raises(ValueError, match="31"):
            fn(31, 30)
        assert fn(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
        assert fn(224, 224) == [(55, 55), (27, 27), (13, 13), (13, 13), (13, 13)]
    for h, w in CASES.E2E_SIZES:
        outs = R.trunk(alex, torch.zeros(1, 3, h, w), torch.float32)
        assert [tuple(o.shape[2:]) for o in outs] == lpips.feature_sizes(h, w)
        assert [o.shape[1] for o in outs] == list(lpips.CHANNELS) == list(R.CHANNELS)
    with pytest.raises(ValueError):
        R.trunk(alex, torch.zeros(1, 3, 30, 31))


def test_state_dict_keys():
    from wu import lpips
    alex, lin = R.make_params(CASES.PARAM_SEED)
    m = lpips.LPIPS()
    assert sorted(m.net.state_dict()) == sorted(alex)
    assert not m.training and not m.net.training and not m.train().training
    m.load_alexnet(alex)
    m.load_alexnet({**alex, "classifier.1.weight": torch.zeros(4096, 9216), "classifier.6.bias": torch.zeros(1000)})
    assert torch.equal(m.net.features.get_submodule("3").weight, alex["features.3.weight"])
    missing = {k: v for k, v in alex.items() if k != "features.8.bias"}
    with pytest.raises(RuntimeError, match="missing"):
        m.load_alexnet(missing)
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_alexnet({**alex, "features.12.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="shape"):
        m.load_alexnet({**alex, "features.0.weight": torch.zeros(64, 3, 3, 3)})
    m.load_lin(lin)
    assert torch.equal(m.lin2.model.get_submodule("1").weight, lin["lin2.model.1.weight"])
    with pytest.raises(RuntimeError, match="missing"):
        m.load_lin({k: v for k, v in lin.items() if not k.startswith("lin4")})
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_lin({**lin, "lin5.model.1.weight": torch.zeros(1, 256, 1, 1)})
    with pytest.raises(RuntimeError, match="shape"):
        m.load_lin({**lin, "lin1.model.1.weight": torch.zeros(192)})
    with pytest.raises(ValueError):
        lpips.LPIPS(precision="fp16")


def test_no_cpu_fallback_and_argument_errors():
    from wu import _lib, lpips
    m = lpips.LPIPS()
    x = torch.zeros(2, 3, 31, 31)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.distance(x, x[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.pairwise(torch.zeros(2, 2, 3, 31, 31))
    with pytest.raises(ValueError):
        lpips.input_mapping((0, 255))
    lib = _lib.load()
    A = 4096                                     # any 16-byte aligned, non-null address: validation happens before anything is dereferenced
    assert lib.wu_lpips_tile_pixels() >= 1
    assert lib.wu_lpips_workspace_bytes(2, 3, 13, 13, 0) > 0 and lib.wu_lpips_workspace_bytes(2, 1, 13, 13, 1) == 0
    assert lib.wu_lpips_head(A, 64, A, 64, 0, A, _lib.F32, 2, 1, 3, 3, 40, A, A, 2, None) < 0 and b"multiple of 16" in lib.wu_last_error()
    assert lib.wu_lpips_head(A, 64, A, 64, 0, A, _lib.F32, 2, 1, 3, 3, 528, A, A, 2, None) < 0
    assert lib.wu_lpips_head(A, 60, A, 64, 0, A, _lib.F32, 2, 1, 3, 3, 48, A, A, 2, None) < 0 and b"ld" in lib.wu_last_error()
    assert lib.wu_lpips_pairs(A, 64, 0, A, _lib.F32, 2, 1, 3, 3, 64, A, A, 2, None) < 0 and b"R" in lib.wu_last_error()
    assert lib.wu_lpips_input(A, 1, 1, 1, 1, 7, 1, 31, 31, 1.0, 0.0, A, _lib.F32, None) < 0


def test_integer_trunk_oracle_is_exact_in_fp32():
    """The operands of the exact trunk test keep every partial sum below 2^24, and the int64 unfolding equals F.conv2d in float64."""
    for case in CASES.TRUNK_CONVS:
        name, n, h, w, cin, cin_w, cout, k, s, p = case
        x, wt, b = CASES.trunk_operands(case)
        want = CASES.trunk_expected(case)
        ref = F.relu(F.conv2d(x[:, :cin_w].double(), wt.double(), b.double(), s, p))
        assert torch.equal(want.double(), ref) and int(want.max()) < 2 ** 24 and (want > 0).any(), name
