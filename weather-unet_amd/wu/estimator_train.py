"""Training step and evaluation pass for the trainable ResNet-101 (wu.resnet_train): the two pre-training jobs of the workflow -- the
5-way weather classifier (classifier.py) and the 5-signal regression estimator (estimator.py) -- on tensors.  Data loading, transforms
and logging stay with the caller (wu.input_pipeline does the transforms on the GPU).

    tr = EstimatorTrainer(resnet101(num_classes=5).cuda(), mode="est")
    for images, signals in batches:
        loss, metrics = tr.step(images, signals)
    tr.save_checkpoint("estimator.pt")                 # a state dict: loads into ResNet101Estimator for the GAN loop

mode "cls" (classifier.py:115-146): cross-entropy loss, Adam with lr 1e-4 and weight decay 1e-4, metric "precision" = the fraction
    of argmax predictions equal to the label.
mode "est" (estimator.py:160-191): squared error per element, averaged over the batch dimension only, back-propagated with a vector of
    ones (so the five per-signal losses are summed); Adam with lr 1e-4 and weight decay 1e-5; metrics "l1_loss" and "adv_loss"
    (ops.l1_loss / ops.adv_loss).
pre_trained=True freezes as the scripts do: for "cls" the whole backbone (only a freshly created fc trains); for "est" the first seven
    children, conv1 .. layer3 (layer4 and a fresh fc train).  The ImageNet weights themselves are a torchvision download and are not
    reproduced here: load a state dict first.

Evaluation runs the model in train mode under no_grad, as the scripts do (they never switch to eval mode): batch statistics, and the
running statistics move.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

MODES = {"cls": {"lr": 1e-4, "weight_decay": 1e-4}, "est": {"lr": 1e-4, "weight_decay": 1e-5}}
FROZEN_CHILDREN_EST = 7         # conv1, bn1, relu, maxpool, layer1, layer2, layer3


def accuracy(outputs, labels):
    """Fraction of rows whose argmax equals the label (the classifier's "precision" metric)."""
    return (outputs.argmax(dim=1) == labels).float().mean()


def freeze_pretrained(model, mode, num_classes):
    """Freeze as the --pre_trained branch of the classifier / estimator script and give the model a new head on the old head's device."""
    dev = model.fc.weight.device
    children = list(model.children())
    frozen = children if mode == "cls" else children[:FROZEN_CHILDREN_EST]
    for child in frozen:
        for p in child.parameters():
            p.requires_grad_(False)
    model.fc = nn.Linear(model.fc.in_features, num_classes).to(dev)
    return model


class EstimatorTrainer:
    def __init__(self, model, mode="est", pre_trained=False, lr=None, weight_decay=None, num_classes=None):
        if mode not in MODES:
            raise ValueError(f"mode must be 'cls' or 'est', got {mode!r}")
        self.mode, self.model = mode, model
        if pre_trained:
            freeze_pretrained(model, mode, num_classes if num_classes is not None else model.fc.out_features)
        cfg = dict(MODES[mode])
        if lr is not None:
            cfg["lr"] = lr
        if weight_decay is not None:
            cfg["weight_decay"] = weight_decay
        # every parameter is handed to Adam, as in the scripts: frozen ones never get a gradient and Adam skips them
        self.opt = torch.optim.Adam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])

    def loss(self, outputs, targets):
        """The training loss and the vector its backward is seeded with (None: a scalar loss)."""
        if self.mode == "cls":
            return F.cross_entropy(outputs, targets), None
        per_signal = F.mse_loss(outputs, targets, reduction="none").mean(dim=0)
        return per_signal, torch.ones_like(per_signal)

    def metrics(self, outputs, targets):
        import ops
        if self.mode == "cls":
            return {"loss": F.cross_entropy(outputs, targets), "precision": accuracy(outputs, targets)}
        return {"l1_loss": ops.l1_loss(outputs, targets), "adv_loss": ops.adv_loss(outputs, targets)}

    def step(self, inputs, targets):
        """One training iteration -> (loss, {metric: value}), all detached tensors."""
        self.model.train()
        self.opt.zero_grad()
        outputs = self.model(inputs)
        loss, seed = self.loss(outputs, targets)
        loss.backward(seed)
        self.opt.step()
        m = self.metrics(outputs.detach(), targets)
        m.pop("loss", None)
        return loss.detach(), m

    def evaluate(self, batches):
        """Mean of each metric over (inputs, targets) batches, train mode under no_grad."""
        self.model.train()
        sums, count = {}, 0
        with torch.no_grad():
            for inputs, targets in batches:
                for k, v in self.metrics(self.model(inputs), targets).items():
                    sums[k] = sums.get(k, 0.0) + v.item()
                count += 1
        return {k: v / count for k, v in sums.items()}

    def save_checkpoint(self, path, with_optimizer=False):
        """The model's state dict (plus the optimizer's on request): loadable without torchvision, into either ResNet-101 module."""
        obj = {"model": self.model.state_dict()}
        if with_optimizer:
            obj["optimizer"] = self.opt.state_dict()
        torch.save(obj, path)

    def load_checkpoint(self, path, strict=True):
        obj = torch.load(path, map_location=self.model.fc.weight.device)
        self.model.load_state_dict(obj["model"], strict=strict)
        if "optimizer" in obj:
            self.opt.load_state_dict(obj["optimizer"])
        return self.model


def load_estimator(path, num_classes=5, precision="bf16"):
    """A checkpoint of ``EstimatorTrainer.save_checkpoint`` -> a frozen ``ResNet101Estimator`` on the CPU (move it to the GPU and hand it
    to ``WeatherTransferStep(estimator=...)``)."""
    from .resnet import ResNet101Estimator
    est = ResNet101Estimator(num_classes, precision=precision)
    est.load_state_dict(torch.load(path, map_location="cpu")["model"], strict=True)
    return est
