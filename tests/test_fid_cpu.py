"""CPU: the host side of FID / Inception Score (wu/fid.py) and the InceptionV3 module's interface (wu/inception.py) without a GPU --
the Frechet distance against closed forms and a straight scipy restatement, the Inception Score against hand-computed values, the
.npz interchange, the state-dict key sets of both variants against tests/_inception_ref.py, strict loading, and the argument checks of
the new C entry points (include/wu_kernels.h, "InceptionV3 forward")."""
import numpy as np
import pytest
import torch

import _inception_ref as R


def _lib():
    from wu import _build, _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib


def test_frechet_distance_diagonal_closed_form():
    from wu.fid import calculate_frechet_distance
    rng = np.random.default_rng(0)
    for d in (1, 8, 64):
        mu1, mu2 = rng.normal(size=d), rng.normal(size=d)
        a, b = rng.uniform(0.2, 3.0, d), rng.uniform(0.2, 3.0, d)
        want = ((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
        got = calculate_frechet_distance(mu1, np.diag(a), mu2, np.diag(b))
        assert abs(got - want) <= 1e-9 * abs(want), (d, got, want)


def test_frechet_distance_matches_a_scipy_restatement_on_spd_pairs():
    from scipy import linalg
    from wu.fid import calculate_frechet_distance
    rng = np.random.default_rng(1)
    for d in (4, 32, 128):
        a, b = rng.normal(size=(d, 2 * d)), rng.normal(size=(d, 2 * d))
        s1, s2 = a @ a.T / (2 * d), b @ b.T / (2 * d) + 0.1 * np.eye(d)
        mu1, mu2 = rng.normal(size=d), rng.normal(size=d)
        want = (mu1 - mu2) @ (mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(linalg.sqrtm(s1 @ s2).real)
        got = calculate_frechet_distance(mu1, s1, mu2, s2)
        assert abs(got - want) <= 1e-10 * abs(want), (d, got, want)


def test_frechet_distance_eps_retry_on_a_singular_product(capsys):
    """sigma1 sigma2 = [[0, 1], [0, 0]] has no square root: sqrtm returns non-finite entries and the eps * I offset is retried (the offset
    product is triangular with eigenvalues (1 + eps) eps and eps^2: a real root).  Positive semi-definite pairs never give a nilpotent
    non-zero product, so the pair is not one; the retry exists for covariances that are singular in floating point."""
    from scipy import linalg
    from wu.fid import calculate_frechet_distance
    s1, s2 = np.array([[1.0, 0.0], [0.0, 0.0]]), np.array([[0.0, 1.0], [0.0, 0.0]])
    mu = np.zeros(2)
    with np.errstate(all="ignore"):
        first, _ = linalg.sqrtm(s1 @ s2, disp=False)
        assert not np.isfinite(first).all()
        eps = 1e-6
        off = np.eye(2) * eps
        cm = linalg.sqrtm((s1 + off) @ (s2 + off))
        got = calculate_frechet_distance(mu, s1, mu, s2, eps=eps)
    assert "adding 1e-06 to diagonal" in capsys.readouterr().out
    want = np.trace(s1) + np.trace(s2) - 2 * np.trace(cm.real)
    assert np.isfinite(got) and abs(got - want) <= 1e-9 * max(1.0, abs(want))


def test_inception_score_hand_computed():
    from wu.fid import inception_score
    p = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.5, 0.5]])
    m, s = inception_score(p, splits=1)
    assert abs(m - np.sqrt(2.0)) < 1e-12 and s == 0.0           # KL = log 2, log 2, 0, 0 -> exp(log(2) / 2)
    m, s = inception_score(p, splits=2)
    assert abs(m - 1.5) < 1e-12 and abs(s - 0.5) < 1e-12        # splits: exp(log 2) = 2 and exp(0) = 1
    logits = torch.tensor([[np.log(3.0), 0.0], [0.0, np.log(3.0)]])
    kl = 0.75 * np.log(1.5) + 0.25 * np.log(0.5)                 # softmax rows (3/4, 1/4), (1/4, 3/4); p(y) = (1/2, 1/2)
    m, s = inception_score(logits, splits=1)
    assert abs(m - np.exp(kl)) < 1e-12 and s == 0.0


def test_statistics_npz_round_trip(tmp_path):
    """finalize() of the shifted fp64 sums equals np.mean / np.cov; save_npz writes fid_score.py's keys and reads back through the CLI path."""
    from wu.fid import FIDStatistics, statistics_of_path
    rng = np.random.default_rng(2)
    x = 5.0 + rng.normal(size=(300, 16))
    k = x[:50].mean(0)
    st = FIDStatistics(None)
    st.n = x.shape[0]
    st._shift = torch.from_numpy(k).float()
    xc = x - st._shift.double().numpy()
    st._sum, st._cross = torch.from_numpy(xc.sum(0)), torch.from_numpy(xc.T @ xc)
    path = str(tmp_path / "stats.npz")
    st.save_npz(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["mu", "sigma"]
    mu, sigma = statistics_of_path(path, None, 50)
    np.testing.assert_allclose(mu, x.mean(0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(sigma, np.cov(x, rowvar=False), rtol=0, atol=1e-12)


@pytest.mark.parametrize("fid", [True, False])
def test_state_dict_keys_match_the_restatement(fid):
    from wu.inception import InceptionV3
    m = InceptionV3(use_fid_inception=fid)                      # constructed on the CPU, no GPU touched
    assert set(m.state_dict()) == set(R.make_params(fid))
    for k, v in R.make_params(fid).items():
        assert tuple(m.state_dict()[k].shape) == tuple(v.shape), k


def test_strict_load_accepts_the_weight_files_and_rejects_missing_or_extra_keys():
    from wu.inception import InceptionV3
    m = InceptionV3()
    m.load_state_dict(R.make_params(True, num_batches_tracked=False))       # pytorch-fid's file may lack num_batches_tracked
    sd = R.make_params(True)
    m.load_state_dict(sd)
    assert torch.equal(m.Mixed_6e.branch7x7dbl_5.conv.weight, sd["Mixed_6e.branch7x7dbl_5.conv.weight"])
    missing = dict(sd)
    del missing["Mixed_7c.branch_pool.bn.running_var"]
    with pytest.raises(RuntimeError, match="Mixed_7c.branch_pool.bn.running_var"):
        m.load_state_dict(missing)
    with pytest.raises(RuntimeError, match="AuxLogits.fc.weight"):
        m.load_state_dict({**sd, "AuxLogits.fc.weight": torch.zeros(1008, 768)})
    with pytest.raises(RuntimeError):
        m.load_state_dict(R.make_params(False))                              # torchvision's fc (1000) into the FID variant
    tv = InceptionV3(use_fid_inception=False)
    tv.load_state_dict({**R.make_params(False), "AuxLogits.fc.weight": torch.zeros(1000, 768)})   # ignored, as documented


def test_module_refuses_what_it_cannot_do():
    from wu.inception import InceptionV3
    with pytest.raises(ValueError, match="forward-only"):
        InceptionV3(requires_grad=True)
    with pytest.raises(ValueError):
        InceptionV3(output_blocks=[4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        InceptionV3()(torch.zeros(1, 3, 299, 299))
    m = InceptionV3(output_blocks=[3], resize_input=False)
    m._check_size(75, 75)
    with pytest.raises(ValueError, match="too small to reach block 3"):
        m._check_size(74, 74)
    InceptionV3(output_blocks=[0], resize_input=False)._check_size(11, 11)
    with pytest.raises(ValueError, match="too small"):
        InceptionV3(output_blocks=[0], resize_input=False)._check_size(10, 200)


def test_new_entry_points_report_argument_errors_without_a_gpu():
    L = _lib()
    lib = L.load()
    conv = lambda cin, cout, kh=3, kw=3, p=1: lib.wu_conv_kxk_fwd(None, 64, None, None, None, 64, 1, 8, 8, cin, cout, kh, kw, 1, 1, p, p,  # noqa: E731
                                                                 L.ACT_RELU, L.F32, None)
    assert conv(64, 40) < 0 and b"Cout" in lib.wu_last_error()
    assert conv(24, 64) < 0 and b"Cin" in lib.wu_last_error()
    assert conv(64, 64, 3, 3, 3) < 0 and b"pad" in lib.wu_last_error()
    assert conv(64, 64) < 0 and b"aligned" in lib.wu_last_error()            # shapes fine, NULL pointers refused
    assert lib.wu_pool3x3_fwd(None, 64, None, 64, 1, 8, 8, 64, 2, 0, 7, L.F32, None) < 0 and b"mode" in lib.wu_last_error()
    assert lib.wu_pool3x3_fwd(None, 64, None, 64, 1, 8, 8, 64, 2, 0, 1, L.F32, None) < 0 and b"average" in lib.wu_last_error()
    assert lib.wu_global_avgpool_fwd(None, 64, None, 64, 1, 8, 8, 66, L.F32, None) < 0 and b"C 66" in lib.wu_last_error()
    assert lib.wu_inception_input(None, 0, 1, 8, 8, 1.0, 0.0, 1, None, 16, 299, 299, 6, L.F32, None) < 0 and b"cpad" in lib.wu_last_error()
    assert lib.wu_feature_stats_update(None, 8, 0, 8, None, 1, None, None, None) < 0 and b"B 0" in lib.wu_last_error()
    assert lib.wu_pack_conv_kxk(None, None, 1000, 3, 16, 1, 1, L.F32, None) < 0 and b"Cout" in lib.wu_last_error()
    # packed size: Cout rounded up to 64 rows, K = 9 * 16 = 144 rounded up to a whole 128-byte step (32 fp32 / 64 bf16)
    assert lib.wu_conv_kxk_packed_bytes(32, 16, 3, 3, L.F32) == 64 * 160 * 4
    assert lib.wu_conv_kxk_packed_bytes(48, 16, 3, 3, L.BF16) == 64 * 192 * 2
