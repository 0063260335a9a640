"""GPU: the shared-encoder condition sweep (Conditional_UNet.sweep, wu/unet_graph.py: unet_sweep) and what is built on it.

Everything is pinned BIT FOR BIT (torch.equal) to the code that existed before the sweep: the kernel to ``wu_adain_upcat_fwd`` on the
materialised repeated inputs, the statistics entry point to ``wu_adain_stats`` on the repeated tensor, the model to the repeated-batch
forward of the unchanged module, the drivers to their per-row loops, the evaluation classes to the reference's loops restated here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, R = 2, 3


def _dev():
    return torch.device("cuda", 0)


def _tdt(p):
    return torch.bfloat16 if p == "bf16" else torch.float32


def _nhwc_rand(n, c, h, w, dt, seed, ld=None):
    """(N,C,H,W)-shaped NHWC tensor of random values; ``ld`` > c: a channel slice of a wider buffer."""
    g = torch.Generator().manual_seed(seed)
    buf = (torch.rand((n, h, w, ld or c), generator=g) * 4 - 2).to(dt).to(_dev())
    return buf.permute(0, 3, 1, 2)[:, :c]


def _stats_rand(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    st = torch.empty(n, c, 2)
    st[..., 0] = torch.rand((n, c), generator=g) - 0.5
    st[..., 1] = torch.rand((n, c), generator=g) + 0.5
    return st.to(_dev()), (torch.rand((n, c), generator=g) + 0.5).to(_dev()), (torch.rand((n, c), generator=g) - 0.5).to(_dev())


# ---------------------------------------------------------------------------------------------------- 1. kernel, through the C ABI
@pytest.mark.parametrize("march", [1, 0])
@pytest.mark.parametrize("p", ["bf16", "fp32"])
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("hw", [(3, 5), (9, 40)])
def test_sweep_kernel_equals_parent_on_repeated_inputs(march, p, c, hw):
    """wu_adain_upcat_sweep_fwd against wu_adain_upcat_fwd on the materialised repeat plus a slice copy of the skip: both source modes
    (Bx = B: one activation shared by all rows; Bx = N), p_drop 0 and 0.3, a host seed and a device-side seed offset, both formulations."""
    from wu import _lib
    from wu.layout import empty_nhwc, nhwc_ld, precision_code, stream_ptr
    h, w = hw
    cs, n, dt, code = 64, R * B, _tdt(p), precision_code(p)
    skip = _nhwc_rand(B, cs, 2 * h, 2 * w, dt, 7, ld=cs + 32)            # a channel slice: its own leading dimension
    _, ystd, ymean = _stats_rand(n, c, 11)
    seed_dev = torch.tensor([12345], dtype=torch.int64, device=_dev())
    _lib.call("wu_set_option", 9, march)
    try:
        for bx in (B, n):
            x = _nhwc_rand(bx, c, h, w, dt, 3 + bx)
            stats = _stats_rand(bx, c, 5 + bx)[0]
            x_rep = x.repeat(n // bx, 1, 1, 1).contiguous(memory_format=torch.channels_last)
            stats_rep = stats.repeat(n // bx, 1, 1).contiguous()
            for p_drop, sd in ((0.0, None), (0.3, None), (0.3, seed_dev)):
                ref = empty_nhwc(n, c + cs, 2 * h, 2 * w, dt, _dev())
                ref.fill_(9.0)
                _lib.call("wu_adain_upcat_fwd", x_rep.data_ptr(), nhwc_ld(x_rep), stats_rep.data_ptr(), ystd.data_ptr(), ymean.data_ptr(),
                          ref.data_ptr(), nhwc_ld(ref), n, h, w, c, p_drop, 77, sd.data_ptr() if sd is not None else None, None, 0,
                          code, stream_ptr())
                ref[:, c:] = skip.repeat(R, 1, 1, 1)
                out = empty_nhwc(n, c + cs, 2 * h, 2 * w, dt, _dev())
                out.fill_(-9.0)
                _lib.call("wu_adain_upcat_sweep_fwd", x.data_ptr(), nhwc_ld(x), bx, stats.data_ptr(), ystd.data_ptr(), ymean.data_ptr(),
                          skip.data_ptr(), nhwc_ld(skip), B, cs, out.data_ptr(), nhwc_ld(out), n, h, w, c, p_drop, 77,
                          sd.data_ptr() if sd is not None else None, code, stream_ptr())
                assert torch.equal(out, ref), (march, p, c, hw, bx, p_drop, sd is not None)
                if p_drop > 0:
                    assert (out[:, :c] == 0).float().mean().item() > 0.2          # the dropout did run
    finally:
        _lib.call("wu_set_option", 9, 1)


# ---------------------------------------------------------------------------------------------------- 2. statistics variant
@pytest.mark.parametrize("p", ["bf16", "fp32"])
def test_stats_with_the_split_count_of_a_stated_batch(p):
    """B=2, C=512, 17x17: wu_adain_stats splits the 289 pixels in 2 for a batch of 2 and in 1 for a batch of 128; the variant computes the
    two images' statistics with the count of 128 -- bit for bit wu_adain_stats on the 128-fold repeat (the plain B=2 call folds in another
    order and is not required to agree)."""
    from wu import kernels as K
    x = _nhwc_rand(2, 512, 17, 17, _tdt(p), 21)
    rep = x.repeat(64, 1, 1, 1).contiguous(memory_format=torch.channels_last)
    ref = K.adain_stats(rep, 1e-5)
    got = K.adain_stats_as_batch(x, 1e-5, 128)
    assert torch.equal(got, ref[:2]) and torch.equal(ref[:2], ref[126:])


# ---------------------------------------------------------------------------------------------------- 3. model
def _net(p, nc=5, seed=0):
    import cunet
    torch.manual_seed(seed)
    return cunet.Conditional_UNet(nc, precision=p).to(_dev())


def _oracle(net, x, rows, max_images, seed=None):
    """The repeated-batch forward of the unchanged module, chunked as sweep() chunks."""
    from wu.unet_graph import sweep_chunks
    b = x.shape[0]
    outs = []
    with torch.no_grad():
        for r0, r1 in sweep_chunks(rows.shape[0], b, max_images):
            if seed is not None:
                net.dropout_seed = seed
            outs.append(net(x.repeat(r1 - r0, 1, 1, 1), rows[r0:r1].repeat_interleave(b, 0)).view(r1 - r0, b, *x.shape[1:]))
    return torch.cat(outs)


@pytest.mark.parametrize("p", ["bf16", "fp32"])
@pytest.mark.parametrize("hw", [(64, 64), (48, 40)])
def test_sweep_equals_repeated_batch_forward(p, hw):
    net = _net(p)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((B, 3, *hw), generator=g) * 2 - 1).to(_dev())
    rows = torch.randn((R, 5), generator=g).to(_dev())
    for train in (False, True):
        net.train(train)
        for max_images in (None, 4):                  # 4 // B = 2 rows per chunk: two chunks
            before = dict(net.sweep_stats)
            net.dropout_seed = 9
            got = net.sweep(x, rows, max_images)
            ref = _oracle(net, x, rows, max_images, seed=9)
            assert got.shape == (R, B, 3, *hw) and got.dtype == torch.float32
            assert torch.equal(got, ref), (p, hw, train, max_images, (got - ref).abs().max().item())
            # the encoder ran once over the B images, the decoder over the R * B pairs
            assert net.sweep_stats["encoder_images"] - before["encoder_images"] == B
            assert net.sweep_stats["decoder_images"] - before["decoder_images"] == R * B
            assert net.sweep_stats["chunks"] - before["chunks"] == (1 if max_images is None else 2)
    net.dropout_seed = None


def test_sweep_level3_statistics_follow_the_virtual_batch():
    """B=2, R=64 at 136x136: level 3 is 17x17 = 289 pixels, wu_adain_stats folds them in 2 splits for B=2 and in 1 for the virtual batch of
    128 -- the smallest shape at which a level-3 statistic computed "as for B" gives other bits than the repeated batch."""
    net = _net("bf16").eval()
    g = torch.Generator().manual_seed(2)
    x = (torch.rand((B, 3, 136, 136), generator=g) * 2 - 1).to(_dev())
    rows = torch.randn((64, 5), generator=g).to(_dev())
    got = net.sweep(x, rows, 128)
    ref = _oracle(net, x, rows, 128)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


# ---------------------------------------------------------------------------------------------------- 5. drivers and bookkeeping
def test_graphed_sweep_replays_the_eager_sweep():
    from wu.graph_infer import GraphedSweep
    net = _net("bf16")
    g = torch.Generator().manual_seed(3)
    x = (torch.rand((B, 3, 64, 64), generator=g) * 2 - 1).to(_dev())
    rows = torch.randn((R, 5), generator=g).to(_dev())
    for train in (False, True):
        net.train(train)
        gs = GraphedSweep(net, B, 64, R, base_seed=21, max_images=4)       # two decoder chunks in the one graph
        first = gs(x, rows, copy_out=True)
        net.dropout_seed = 21
        assert torch.equal(first, net.sweep(x, rows, 4)), train
        if train:
            second = gs(x, rows, copy_out=True)                            # the graph bumped its own counter: the masks of seed 22
            net.dropout_seed = 22
            assert not torch.equal(second, first) and torch.equal(second, net.sweep(x, rows, 4))
            gs.set_seed_offset(0)
            assert torch.equal(gs(x, rows, copy_out=True), first)
        else:
            assert torch.equal(gs(x, rows, copy_out=True), first)
        net.dropout_seed = None


def test_drivers_with_shared_encoder_equal_their_loops():
    from wu import infer_driver as D
    from wu.graph_infer import GraphedSweep
    net = _net("bf16").eval()
    g = torch.Generator().manual_seed(4)
    x = (torch.rand((B, 3, 64, 64), generator=g) * 2 - 1).to(_dev())
    ref = D.class_sweep(net, x)
    assert torch.equal(D.class_sweep(net, x, shared_encoder=True), ref)
    assert torch.equal(D.class_sweep(net, x, shared_encoder=True, max_images=4), ref)
    assert torch.equal(D.class_sweep(net, x, normalize=True, shared_encoder=True), D.class_sweep(net, x, normalize=True))
    assert torch.equal(D.class_sweep(net, x, shared_encoder=True, graphed=GraphedSweep(net, B, 64, 5)), ref)
    with pytest.raises(ValueError):
        from wu.graph_infer import GraphedUNet
        D.class_sweep(net, x, shared_encoder=True, graphed=GraphedUNet(net, B, 64))
    pred = torch.randn((B, 5), generator=g).to(_dev())
    thetas = (0.3, 1.1)
    assert torch.equal(D.axis_sweep(net, x, pred, thetas, shared_encoder=True), D.axis_sweep(net, x, pred, thetas))
    # one image under 5 rows: the encoder runs for ONE image
    signals = torch.randn((5, 5), generator=g).to(_dev())
    before = dict(net.sweep_stats)
    got = D.image_rows(net, x[0], signals)
    assert net.sweep_stats["encoder_images"] - before["encoder_images"] == 1
    assert net.sweep_stats["decoder_images"] - before["decoder_images"] == 5
    assert torch.equal(got, D.transfer_rows(net, x[:1].repeat(5, 1, 1, 1), signals))


def test_signal_sweep_shared_encoder_where_the_split_count_depends_on_the_batch():
    """B=2, 64 rows at 136x136: the level-3 statistics fold 2 partial sums at batch 2 and 1 at batch 128, so the repeated-batch form need not
    equal 64 separate calls; the driver's default (one row per decoder chunk) does, bit for bit, also with dropout active."""
    from wu import infer_driver as D
    net = _net("bf16")
    g = torch.Generator().manual_seed(8)
    x = (torch.rand((B, 3, 136, 136), generator=g) * 2 - 1).to(_dev())
    rows = torch.randn((64, 5), generator=g).to(_dev())
    for train in (False, True):
        net.train(train)
        net.dropout_seed = 3
        ref = D.signal_sweep(net, x, rows)
        before = dict(net.sweep_stats)
        assert torch.equal(D.signal_sweep(net, x, rows, shared_encoder=True), ref), train
        assert net.sweep_stats["encoder_images"] - before["encoder_images"] == B and net.sweep_stats["chunks"] - before["chunks"] == 64
    net.dropout_seed = None


def test_evaluation_with_shared_encoder_equals_the_default():
    from wu.train_step import WeatherTransferStep
    step = WeatherTransferStep(num_classes=5, mode="est", device=_dev())
    step.inference.eval()
    step.discriminator.eval()
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((4, 3, 64, 64), generator=g) * 2 - 1).to(_dev())
    labels, ref_labels = torch.randn((4, 5), generator=g).to(_dev()), torch.randn((4, 5), generator=g).to(_dev())
    for max_images in (1024, 8):                                           # one chunk; two chunks of two rows
        l0, f0 = step.evaluation(x, labels, ref_labels, max_images)
        l1, f1 = step.evaluation(x, labels, ref_labels, max_images, shared_encoder=True)
        assert torch.equal(f0, f1)
        for k in l0:
            assert torch.equal(l0[k], l1[k]), k


# ---------------------------------------------------------------------------------------------------- 6. evaluation suite
def _eval_setup(b, estimator):
    net = _net("bf16").eval()
    est = estimator.to(_dev()).eval()
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand((b, 3, 64, 64), generator=g) * 2 - 1).to(_dev()) for _ in range(2)]
    refs = [torch.randn((b, 5), generator=g).to(_dev()) for _ in range(2)]
    return net, est, batches, refs


def _check_evaluation(b, estimator):
    """ClassTransferEval / EstimatorTransferEval against the reference's loops (eval_class_transfer.py:112-121, eval_estimator_transfer.py:49-57)
    restated with today's API: per row a full forward of the batch, then the network, then arg-max / the batch mean of pred - row."""
    from wu.evaluate import ClassTransferEval, EstimatorTransferEval
    nc = 5
    net, est, batches, refs = _eval_setup(b, estimator)
    cte, ete = ClassTransferEval(net, est, nc), EstimatorTransferEval(net, est)
    cm = np.zeros((nc, nc), dtype=np.int64)
    rows = []
    eye = torch.eye(nc, device=_dev())
    with torch.no_grad():
        for batch, ref in zip(batches, refs):
            cte.update(batch)
            ete.update(batch, ref)
            for i in range(nc):
                out = net(batch, eye[i].unsqueeze(0).expand(b, nc).contiguous())
                for pred in est(out).float().argmax(1).tolist():
                    cm[i, pred] += 1
            for j in range(ref.shape[0]):
                expand = ref[j].unsqueeze(0).expand(b, nc).contiguous()
                rows.append((est(net(batch, expand)).float() - expand).mean(0).cpu().numpy())
    got_cm = cte.confusion()
    assert got_cm.dtype == torch.int64 and got_cm.sum().item() == 2 * nc * b
    assert np.array_equal(got_cm.cpu().numpy(), cm), (got_cm, cm)
    assert cte.report()["accuracy"] == pytest.approx(np.trace(cm) / cm.sum())
    rows = np.stack(rows).astype(np.float64)
    res = ete.result()
    assert res["count"] == rows.shape[0] == 2 * b
    # The generator outputs are bit-identical; the estimator sees them in passes of R * B instead of B images.  Its outputs are O(1) fp32
    # numbers from dot products whose summation order a GEMM may choose by batch size: a few fp32 ulps (2^-23 = 1.2e-7 at 1), far below 1e-5;
    # a wrong row, a wrong sign or a sample std would be off by O(0.1).
    scale = max(1.0, float(np.abs(rows).max()))
    d_mean = float(np.abs(res["mean"].cpu().numpy() - rows.mean(0)).max())
    d_std = float(np.abs(res["std"].cpu().numpy() - rows.std(0)).max())
    print(f"EstimatorTransferEval vs numpy on the looped rows: mean {d_mean:.3e} std {d_std:.3e} (scale {scale:.2f})")
    assert d_mean <= 1e-5 * scale and d_std <= 1e-5 * scale


def test_evaluation_suite_against_the_reference_loops():
    from wu.train_step import StandInEstimator
    torch.manual_seed(11)
    _check_evaluation(4, StandInEstimator(5))


def test_evaluation_suite_with_the_resnet_estimator():
    from wu.resnet import ResNet101Estimator
    torch.manual_seed(12)
    _check_evaluation(2, ResNet101Estimator(5, layers=((64, 1, 1), (128, 1, 2), (256, 1, 2), (512, 1, 2))))
