"""CPU: the trainable ResNet-101's module tree (wu/resnet_train.py) and the training-step glue (wu/estimator_train.py).  No kernel runs."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import resnet_ref as R

TORCHVISION_CHILDREN = ["conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool", "fc"]


def _expected_keys(nc):
    shapes = dict(R.resnet101_param_shapes(nc))
    out = []
    for k, v in shapes.items():
        out.append((k, v))
        if k.endswith("running_var"):
            out.append((k[:-len("running_var")] + "num_batches_tracked", ()))
    return out


def test_state_dict_keys_shapes_and_order_are_torchvisions():
    from wu.resnet_train import resnet101
    m = resnet101(num_classes=5)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _expected_keys(5)
    assert m.state_dict()["bn1.num_batches_tracked"].dtype == torch.long


def test_children_in_torchvision_order_and_trainable():
    from wu.resnet_train import resnet101
    m = resnet101(num_classes=7, precision="fp32")
    assert [n for n, _ in m.named_children()] == TORCHVISION_CHILDREN
    assert all(p.requires_grad for p in m.parameters())
    assert m.fc.in_features == 2048 and m.fc.out_features == 7
    for name in ("relu", "maxpool", "avgpool"):
        assert not list(getattr(m, name).parameters())


def test_state_dict_round_trips_with_the_frozen_estimator():
    from wu.resnet import ResNet101Estimator
    from wu.resnet_train import resnet101
    m = resnet101(num_classes=5)
    est = ResNet101Estimator(5)
    est.load_state_dict(m.state_dict(), strict=True)
    back = resnet101(num_classes=5)
    back.load_state_dict(est.state_dict(), strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k


def test_train_eval_toggle_and_estimator_stays_frozen():
    from wu.resnet import ResNet101Estimator
    from wu.resnet_train import resnet101
    m = resnet101()
    assert m.training
    m.eval()
    assert not m.training and not m.layer3[5].training
    m.train()
    assert m.training and m.layer3[5].training
    est = ResNet101Estimator(5)
    est.train()
    assert not est.training


def test_module_refuses_cpu_tensors():
    from wu.resnet_train import resnet101
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resnet101()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError):
        resnet101(precision="fp16")


def test_pretrained_freezing_selects_the_scripts_parameters():
    from wu.estimator_train import freeze_pretrained
    from wu.resnet_train import resnet101
    m = freeze_pretrained(resnet101(num_classes=5), "cls", 5)
    assert {n for n, p in m.named_parameters() if p.requires_grad} == {"fc.weight", "fc.bias"}
    m = freeze_pretrained(resnet101(num_classes=5), "est", 5)
    train = {n for n, p in m.named_parameters() if p.requires_grad}
    assert train == {n for n, _ in m.named_parameters() if n.startswith(("layer4.", "fc."))}
    assert "layer3.22.bn3.weight" not in train and "layer4.0.downsample.0.weight" in train


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.body = nn.Linear(6, 8)
        self.fc = nn.Linear(8, 5)

    def forward(self, x):
        return self.fc(torch.relu(self.body(x)))


def _clone(m):
    c = _Tiny()
    c.load_state_dict(m.state_dict())
    return c


@pytest.mark.parametrize("mode", ["cls", "est"])
def test_step_glue_matches_the_reference_formulas(mode):
    """EstimatorTrainer.step on a tiny CPU module against the loops written out by hand: the loss, its backward seed, the metrics and
    Adam(lr=1e-4, weight_decay=1e-4 for cls / 1e-5 for est)."""
    import ops
    from wu.estimator_train import EstimatorTrainer
    torch.manual_seed(0)
    m = _Tiny()
    ref = _clone(m)
    tr = EstimatorTrainer(m, mode=mode)
    wd = 1e-4 if mode == "cls" else 1e-5
    g = tr.opt.param_groups[0]
    assert g["lr"] == 1e-4 and g["weight_decay"] == wd and isinstance(tr.opt, torch.optim.Adam)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4, weight_decay=wd)
    for it in range(3):
        x = torch.randn(4, 6)
        t = torch.randint(0, 5, (4,)) if mode == "cls" else torch.rand(4, 5)
        loss, met = tr.step(x, t)
        opt.zero_grad()
        out = ref(x)
        if mode == "cls":
            want = nn.CrossEntropyLoss()(out, t)
            want.backward()
            acc = (torch.argmax(out, 1) == t).float().mean()
            assert torch.equal(met["precision"], acc)
        else:
            want = torch.mean(nn.MSELoss(reduction="none")(out, t), dim=0)
            want.backward(torch.ones(5))
            assert torch.equal(met["l1_loss"], ops.l1_loss(out.detach(), t))
            assert torch.equal(met["adv_loss"], ops.adv_loss(out.detach(), t))
        opt.step()
        assert torch.allclose(loss, want.detach(), rtol=1e-6, atol=0)
        for a, b in zip(m.parameters(), ref.parameters()):
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)


def test_evaluate_averages_over_batches_in_train_mode():
    from wu.estimator_train import EstimatorTrainer
    torch.manual_seed(1)
    m = _Tiny()
    tr = EstimatorTrainer(m, mode="est")
    m.eval()
    batches = [(torch.randn(3, 6), torch.rand(3, 5)) for _ in range(3)]
    res = tr.evaluate(batches)
    assert m.training
    with torch.no_grad():
        want = sum(F.mse_loss(m(x), t).item() for x, t in batches) / 3
    assert abs(res["adv_loss"] - want) <= 1e-6 and set(res) == {"adv_loss", "l1_loss"}


def test_checkpoint_round_trip_into_the_estimator(tmp_path):
    from wu.estimator_train import EstimatorTrainer, load_estimator
    from wu.resnet_train import resnet101
    m = resnet101(num_classes=5)
    with torch.no_grad():
        m.layer2[1].bn2.running_mean.add_(0.5)
    tr = EstimatorTrainer(m, mode="est")
    path = str(tmp_path / "est.pt")
    tr.save_checkpoint(path, with_optimizer=True)
    est = load_estimator(path, 5)
    assert torch.equal(est.layer2[1].bn2.running_mean, m.layer2[1].bn2.running_mean)
    m2 = resnet101(num_classes=5)
    EstimatorTrainer(m2, mode="est").load_checkpoint(path)
    assert torch.equal(m2.fc.weight, m.fc.weight)


def test_abi_entry_points_are_declared():
    from wu import _lib
    for name in ("wu_bn_stats", "wu_bn_apply", "wu_bn_bwd", "wu_conv1x1_wgrad", "wu_stem7x7_wgrad", "wu_bn_stats_workspace",
                 "wu_bn_bwd_workspace", "wu_conv1x1_wgrad_workspace", "wu_stem7x7_wgrad_workspace"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.wu_conv1x1_wgrad_workspace(100, 48, 64) == 0 and lib.wu_conv1x1_wgrad_workspace(100, 64, 64) > 0
    assert lib.wu_bn_stats_workspace(784, 2048, _lib.BF16) > 0 and lib.wu_stem7x7_wgrad_workspace(2, 61, 47) > 0
    rc = lib.wu_bn_stats(None, 64, 10, 40, 1e-5, 0.1, None, None, None, None, None, 0, _lib.BF16, None)
    assert rc < 0 and b"bn_stats" in lib.wu_last_error()
