"""InceptionV3 / FID on the GPU (csrc/inception.hip, wu/inception.py, wu/fid.py) against the float64 CPU restatement
tests/_inception_ref.py (torch.nn.functional ops, written from the architecture; torchvision is not importable here).
bf16 cases compare against float64 results of bf16-rounded operands where a single kernel is tested.
Everything here runs at the shapes of a square 299 x 299 network input; tests/test_gpu_inception_edges.py covers H != W, channel slices,
the batch split, small pool maps, ragged feature batches and the conv's exact integer oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _inception_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "weather-unet_amd")


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _cos(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return (torch.dot(a, b) / (a.norm() * b.norm())).item()


def _tdt(p):
    return torch.float32 if p == "fp32" else torch.bfloat16


def _nhwc(x, dtype):
    """(N, C, H, W) CPU tensor -> NHWC-strided GPU tensor of `dtype`."""
    return x.to(dtype).permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)


def _conv_shapes():
    seen, out = set(), []
    for name, cin, cout, k, s, p in R.CONVS:
        key = (k[0], k[1], s, p, cin, cout, R.input_size(name))
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out


def _run_conv(x_nhwc, w, b, y, k, s, p, cin_w=None):
    from wu import _lib
    from wu.inception import conv_kxk
    from wu.layout import dtype_code
    code = dtype_code(x_nhwc)
    cout, cw = w.shape[0], w.shape[1]
    cin = x_nhwc.shape[1]
    nbytes = _lib.load().wu_conv_kxk_packed_bytes(cout, cin, k[0], k[1], code)
    wp = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    wd = w.float().contiguous().to(DEV)
    _lib.call("wu_pack_conv_kxk", wd.data_ptr(), wp.data_ptr(), cout, cw, cin, k[0], k[1], code, torch.cuda.current_stream().cuda_stream)
    p_ = {"w": wp, "b": b.float().contiguous().to(DEV), "k": k, "s": (s, s), "p": p, "cout": cout, "code": code}
    return conv_kxk(x_nhwc, p_, y)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_kernel_every_network_shape(prec):
    """Every distinct (KH, KW, stride, pad, Cin, Cout, H) of the network at B = 2 against F.conv2d + bias + ReLU in float64."""
    from wu.layout import empty_nhwc
    g = torch.Generator().manual_seed(0)
    dt = _tdt(prec)
    worst = 0.0
    for kh, kw, s, p, cin, cout, h in _conv_shapes():
        cin_k = 16 if cin == 3 else cin                       # the image's 3 channels arrive zero-padded to 16
        x = torch.randn(2, cin, h, h, generator=g)
        w = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        b = 0.1 * torch.randn(cout, generator=g)
        xr, wr = x.to(dt).double(), w.to(dt).double()
        want = F.relu(F.conv2d(xr, wr, b.double(), s, p))
        xk = torch.zeros(2, cin_k, h, h)
        xk[:, :cin] = x
        y = empty_nhwc(2, cout, want.shape[2], want.shape[3], dt, DEV)
        _run_conv(_nhwc(xk, dt), w, b, y, (kh, kw), s, p)
        err = _rel(y.float(), want)
        worst = max(worst, err)
        assert err <= (1e-5 if prec == "fp32" else 1e-2), ((kh, kw, s, p, cin, cout, h), err)
    print(f"conv {prec}: worst relative L2 {worst:.2e} over {len(_conv_shapes())} shapes")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_reads_and_writes_channel_slices_only(prec):
    """Input and output as channel slices of wider buffers; a sentinel-filled output shows nothing outside [c0, c0 + Cout) is written."""
    g = torch.Generator().manual_seed(1)
    dt = _tdt(prec)
    for (kh, kw, s, p, cin, cout, h) in ((1, 7, 1, (0, 3), 48, 80, 17), (3, 3, 2, (0, 0), 32, 48, 35), (1, 1, 1, (0, 0), 64, 32, 9)):
        big = torch.randn(2, cin + 48, h, h, generator=g)
        x = _nhwc(big, dt)[:, 16:16 + cin]
        w = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        b = 0.1 * torch.randn(cout, generator=g)
        want = F.relu(F.conv2d(big[:, 16:16 + cin].to(dt).double(), w.to(dt).double(), b.double(), s, p))
        ho, wo = want.shape[2], want.shape[3]
        ctot = cout + 64
        out = torch.full((2, ho, wo, ctot), 7.0, dtype=dt, device=DEV).permute(0, 3, 1, 2)
        _run_conv(x, w, b, out[:, 32:32 + cout], (kh, kw), s, p)
        o = out.float().cpu()
        assert torch.all(o[:, :32] == 7.0) and torch.all(o[:, 32 + cout:] == 7.0)
        assert _rel(o[:, 32:32 + cout], want) <= (1e-5 if prec == "fp32" else 1e-2)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_pools_against_torch(prec):
    from wu.inception import POOL_AVG, POOL_AVG_EXCL_PAD, POOL_MAX, global_avgpool, pool3x3
    from wu.layout import empty_nhwc, precision_code
    code, dt = precision_code(prec), _tdt(prec)
    g = torch.Generator().manual_seed(2)
    for h, c in ((147, 64), (35, 288), (17, 768), (8, 2048)):
        x = torch.randn(2, c, h, h, generator=g).to(dt)
        xd = _nhwc(x, dt)
        xf = x.float()
        for stride, pad, mode in ((2, 0, POOL_MAX), (1, 1, POOL_MAX), (1, 1, POOL_AVG), (1, 1, POOL_AVG_EXCL_PAD)):
            ho = (h + 2 * pad - 3) // stride + 1
            y = pool3x3(xd, empty_nhwc(2, c, ho, ho, dt, DEV), stride, pad, mode, code).float().cpu()
            if mode == POOL_MAX:
                assert torch.equal(y, F.max_pool2d(xf, 3, stride, pad)), (h, c, stride, pad)      # bit-identical
            else:
                want = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=(mode == POOL_AVG))
                if prec == "fp32":
                    assert (y.double() - want).abs().max().item() <= 1e-6 * want.abs().max().item(), (h, c, mode)
                else:
                    assert _rel(y, want) <= 4e-3
        feat = global_avgpool(xd, code).cpu()
        want = x.double().mean(dim=(2, 3))
        assert (feat.double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()


@pytest.mark.parametrize("size", [256, 299, 512])
@pytest.mark.parametrize("src", ["fp32", "u8"])
def test_input_kernel_against_interpolate(size, src):
    """uint8 / fp32 images -> F.interpolate(299, bilinear, align_corners=False) -> 2x - 1, NHWC padded to 16 channels, to 1e-6."""
    from wu.inception import InceptionV3
    g = torch.Generator().manual_seed(size)
    if src == "u8":
        u8 = torch.randint(0, 256, (2, size, size, 3), generator=g, dtype=torch.uint8)
        x01 = torch.from_numpy(u8.numpy().astype(np.float32) / 255).permute(0, 3, 1, 2)      # np.float32 division, as fid_score.py
        inp = u8.to(DEV)
    else:
        x01 = torch.rand(2, 3, size, size, generator=g)
        inp = x01.to(DEV)
    want = R.prepare(x01)
    m = InceptionV3()
    got = m.prepare(inp).float().cpu()
    assert got.shape == (2, 16, 299, 299)
    assert torch.all(got[:, 3:] == 0)
    assert (got[:, :3].double() - want).abs().max().item() <= 1e-6
    # the generator's [-1, 1] range through the affine
    if src == "fp32":
        got = m.prepare((x01 * 2 - 1).to(DEV), value_range=(-1, 1)).float().cpu()
        assert (got[:, :3].double() - want).abs().max().item() <= 2e-6


def _images(n, seed, size=64):
    """Smooth random fields in [0, 1]: 4 x 4 random colour grids, bilinear to size x size."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(n, 3, 4, 4, generator=g)
    return F.interpolate(coarse, size=(size, size), mode="bilinear", align_corners=False).clamp(0, 1)


@pytest.mark.parametrize("fid", [True, False])
def test_whole_network_blocks_and_logits(fid):
    from wu.inception import InceptionV3
    sd = R.make_params(fid, seed=3)
    x01 = _images(2, 4, 96)
    ref = R.forward(sd, R.prepare(x01), fid)
    for prec in ("fp32", "bf16"):
        m = InceptionV3(output_blocks=[0, 1, 2, 3], use_fid_inception=fid, precision=prec)
        m.load_state_dict(sd)
        outs = m(x01.to(DEV))
        logits = m.logits(x01.to(DEV))
        assert [tuple(o.shape) for o in outs] == [(2, 64, 73, 73), (2, 192, 35, 35), (2, 768, 17, 17), (2, 2048, 1, 1)]
        assert tuple(logits.shape) == (2, R.num_classes(fid))
        errs = [_rel(outs[i].float().reshape(2, -1) if i < 3 else outs[i].reshape(2, -1), ref[i].reshape(2, -1)) for i in range(4)]
        errs.append(_rel(logits, ref["logits"]))
        coss = [_cos(outs[i].float(), ref[i]) for i in range(4)] + [_cos(logits, ref["logits"])]
        print(f"fid={fid} {prec}: relative L2 per block + logits {['%.2e' % e for e in errs]}, cosine {['%.6f' % c for c in coss]}")
        if prec == "fp32":
            assert max(errs) <= 1e-4, errs
        else:
            assert min(coss) >= 0.999, coss


def test_feature_statistics_against_numpy():
    from wu.fid import FIDStatistics
    rng = np.random.default_rng(5)
    d = 2048
    rows = (3.0 + rng.normal(size=(1000, d)) * rng.uniform(0.1, 2.0, d)).astype(np.float32)
    st = FIDStatistics(None)
    for i in range(0, 1000, 50):
        st.update_features(torch.from_numpy(rows[i:i + 50]).to(DEV))
    mu, sigma = st.finalize()
    r = rows.astype(np.float64)
    want_s = np.cov(r, rowvar=False)
    assert np.abs(mu - r.mean(0)).max() <= 1e-6 * np.abs(r.mean(0)).max()
    assert np.abs(sigma - want_s).max() <= 1e-6 * np.abs(want_s).max(), np.abs(sigma - want_s).max() / np.abs(want_s).max()


def test_fid_end_to_end_and_cli(tmp_path):
    """dims = 64: two seeded sets of 128 smooth images (the second colour-shifted) through the GPU path against FID from the float64
    restatement's features + np.cov, then the same value through `python -m wu.fid` on PNG directories (child process, timeout)."""
    from PIL import Image
    from wu.fid import FIDStatistics, calculate_frechet_distance
    from wu.inception import InceptionV3
    sd = R.make_params(True, seed=6)
    base = _images(128, 7)
    shift = torch.tensor([0.15, -0.1, 0.05]).view(1, 3, 1, 1)
    sets_u8 = [(x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() for x in (base, (base + shift).clamp(0, 1))]
    model = InceptionV3([0])
    model.load_state_dict(sd)
    gpu_stats, ref_stats = [], []
    for u8 in sets_u8:
        st = FIDStatistics(model)
        for i in range(0, 128, 50):
            st.update(u8[i:i + 50].to(DEV))
        gpu_stats.append(st.finalize())
        x01 = torch.from_numpy(u8.numpy().astype(np.float32) / 255).permute(0, 3, 1, 2)
        feats = torch.cat([R.forward(sd, R.prepare(x01[i:i + 16]), True, last=0)[0].mean(dim=(2, 3)) for i in range(0, 128, 16)]).numpy()
        ref_stats.append((feats.mean(0), np.cov(feats, rowvar=False)))
    fid_gpu = calculate_frechet_distance(*gpu_stats[0], *gpu_stats[1])
    fid_ref = calculate_frechet_distance(*ref_stats[0], *ref_stats[1])
    print(f"FID dims=64: GPU {fid_gpu:.8f} float64 reference {fid_ref:.8f}")
    assert fid_ref > 0 and abs(fid_gpu - fid_ref) <= 1e-3 * fid_ref

    dirs = []
    for k, u8 in enumerate(sets_u8):
        d = tmp_path / f"set{k}"
        d.mkdir()
        for i in range(u8.shape[0]):
            Image.fromarray(u8[i].numpy()).save(d / f"img_{i:04d}.png")
        dirs.append(str(d))
    weights = str(tmp_path / "weights.pth")
    torch.save(sd, weights)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "wu.fid", dirs[0], dirs[1], "--weights", weights, "--dims", "64", "--batch-size", "50"],
                       cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("FID: ")]
    assert line, r.stdout[-2000:]
    fid_cli = float(line[-1].split()[1])
    assert abs(fid_cli - fid_ref) <= 1e-3 * fid_ref


def test_features_and_statistics_are_deterministic():
    from wu.fid import FIDStatistics
    from wu.inception import InceptionV3
    sd = R.make_params(True, seed=8)
    x = _images(4, 9, 80).to(DEV)
    runs = []
    for _ in range(2):
        m = InceptionV3([3])
        m.load_state_dict(sd)
        feat = m(x)[0].clone()
        st = FIDStatistics(m)
        st.update(x)
        st.update(x.flip(3))
        runs.append((feat.cpu(), *st.finalize()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
