"""The dataset evaluation of the reference's ``eval/eval_*.py`` on top of the shared-encoder sweep (``Conditional_UNet.sweep``).

* ``ClassTransferEval``      eval_class_transfer.py:106-136    every test image transferred to every class, the classifier's arg-max against
                                                               the target class: confusion matrix + classification report
* ``EstimatorTransferEval``  eval_estimator_transfer.py:48-61,129-130   every image transferred to every reference signal row, the estimator's
                                                               prediction minus the row, averaged per row: mean / std of those errors
* ``ClassifierEval``         eval_classifier_i2w.py:85-106     the classifier on the photographs themselves (no generator)
* ``EstimatorEval``          eval_estimator.py:141-159         the estimator on the photographs themselves: mean / std of pred - target, MSE
* ``ContentPreservation``    (no counterpart in the reference) SSIM / MS-SSIM / MSE / PSNR / MAE between every image and its transferred versions,
                                                               per row; the two transfer evaluations feed it through ``content=``
* ``SlicedWasserstein``      (no counterpart in the reference) the sliced Wasserstein distance on Laplacian-pyramid patches (``wu.swd``) between
                                                               the photographs and their transferred versions, per pyramid level; fed
                                                               through ``swd=``
* ``PerceptualDistance``     (no counterpart in the reference) LPIPS (``wu.lpips``) between every image and its transferred versions, per row,
                                                               and the pairwise-diversity score among the rows; fed through ``lpips=``
* ``SpectralDiscrepancy``    (no counterpart in the reference) the radial power spectrum (``wu.spectrum``) of the photographs against their
                                                               transferred versions: log-spectral distance, band differences and the
                                                               largest single-bin difference, per row; fed through ``spectrum=``

No pandas, plotting or path conventions: callers feed batches (e.g. from ``wu.data.JpegBatchLoader``).  Every ``update`` accumulates on the
device and never synchronises with the host; ``confusion`` / ``report`` / ``result`` read the accumulators back.  The generator and the
networks run in whatever train / eval mode they are in (the reference's scripts leave the generator's Dropout active and call ``.eval()`` on
the classifier / estimator).  Not a hot path: torch arithmetic on a few numbers per image; the kernels behind it are ``wu.paired``'s, ``wu.swd``'s and ``wu.lpips``'s.
"""
import torch

from .unet_graph import SWEEP_MAX_IMAGES


def classification_report(confusion, names=None):
    """``sklearn.metrics.classification_report(y_true, y_pred, output_dict=True)`` from a confusion matrix (rows = true class, columns =
    predicted class): per class ``precision`` / ``recall`` / ``f1-score`` / ``support``, then ``accuracy``, ``macro avg`` and ``weighted avg``.
    sklearn's conventions: an undefined ratio (a class never predicted, or without samples) counts as 0; only the classes that occur in
    y_true or y_pred are listed and averaged; ``macro avg`` is the plain mean over them, ``weighted avg`` weighs by support."""
    cm = torch.as_tensor(confusion).detach().to("cpu", torch.float64)
    if cm.dim() != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"classification_report: a square confusion matrix, got {tuple(cm.shape)}")
    nc = cm.shape[0]
    names = [str(i) for i in range(nc)] if names is None else [str(n) for n in names]
    tp, support, predicted = cm.diag(), cm.sum(1), cm.sum(0)

    def ratio(a, b):
        return torch.where(b > 0, a / b.clamp(min=1), torch.zeros_like(a))

    prec, rec = ratio(tp, predicted), ratio(tp, support)
    f1 = ratio(2 * prec * rec, prec + rec)
    present = [i for i in range(nc) if support[i] > 0 or predicted[i] > 0]
    total = support.sum()
    out = {names[i]: {"precision": prec[i].item(), "recall": rec[i].item(), "f1-score": f1[i].item(), "support": int(support[i].item())}
           for i in present}
    idx = torch.tensor(present, dtype=torch.long)
    out["accuracy"] = (tp.sum() / total).item() if total > 0 else 0.0
    for key, wgt in (("macro avg", torch.ones(len(present), dtype=torch.float64)), ("weighted avg", support[idx])):
        wsum = wgt.sum()
        avg = (lambda v: ((v[idx] * wgt).sum() / wsum).item() if wsum > 0 else 0.0)
        out[key] = {"precision": avg(prec), "recall": avg(rec), "f1-score": avg(f1), "support": int(total.item())}
    return out


class _Confusion:
    """int64 nc x nc counts on the device; rows = true / target class, columns = predicted class."""

    def __init__(self, num_classes, names=None):
        self.num_classes, self.names = int(num_classes), names
        self.cm = None

    def add(self, true_idx, pred_idx):
        nc = self.num_classes
        if self.cm is None:
            self.cm = torch.zeros((nc, nc), dtype=torch.int64, device=pred_idx.device)
        flat = true_idx.to(device=pred_idx.device, dtype=torch.int64) * nc + pred_idx.to(torch.int64)
        self.cm.view(-1).index_add_(0, flat, torch.ones_like(flat))           # no host read, unlike bincount's size query

    def confusion(self):
        nc = self.num_classes
        return self.cm.clone() if self.cm is not None else torch.zeros((nc, nc), dtype=torch.int64)

    def report(self):
        return classification_report(self.confusion(), self.names)


class _Rows:
    """Rows of fp32 numbers appended on the device; mean / population std / mean square over all of them in fp64 (np.mean / np.std)."""

    def __init__(self):
        self.rows = []

    def add(self, r):
        self.rows.append(r.detach().float().reshape(-1, r.shape[-1]))

    def all(self):
        if not self.rows:
            raise RuntimeError("no batch has been added yet")
        return torch.cat(self.rows).double()

    def result(self, mse=False):
        a = self.all()
        out = {"mean": a.mean(0), "std": a.std(0, unbiased=False), "count": a.shape[0]}
        if mse:
            out["mse"] = (a * a).mean(0)
        return out


def _batched(net, images, max_images):
    """net over (M, 3, H, W) in passes of at most ``max_images`` images -> (M, k) fp32."""
    return torch.cat([net(images[i:i + max_images]).float() for i in range(0, images.shape[0], max_images)])


class ContentPreservation:
    """Is it still the same scene?  The paired metrics of ``wu.paired`` (SSIM, MS-SSIM, MSE / PSNR, MAE) between a batch and its R conditioned
    outputs, accumulated per row over a data set.  ``add(batch, fakes)``: batch (B, C, H, W), fakes (R, B, C, H, W) as ``sweep`` returns them
    (R fixed across calls); one fused call per batch, sums kept in fp64 on the device, no host synchronisation.  ``result()``: per row (R,)
    fp64 CPU tensors ``ssim``, ``ms_ssim`` (None with ms=False), ``mse``, ``mae`` -- means over all images -- ``psnr = 10 log10(L^2 / mean
    MSE)`` and the image ``count``.  ms=True needs min(H, W) > 16 (win_size - 1): a ValueError otherwise, never a silent clamp."""

    def __init__(self, ms=True, value_range=(-1, 1), win_size=11):
        self.ms, self.value_range, self.win_size = bool(ms), value_range, int(win_size)
        self.sums, self.count, self.data_range = None, 0, None

    @torch.no_grad()
    def add(self, batch, fakes):
        from . import paired
        if fakes.dim() != 5:
            raise ValueError(f"ContentPreservation.add: fakes must be (R, B, C, H, W), got {tuple(fakes.shape)}")
        st = paired.pair_stats(batch, fakes, self.value_range, self.win_size, levels=paired.MS_LEVELS if self.ms else 1)
        cols = [paired.combine_ssim(st), paired.combine_ms_ssim(st) if self.ms else torch.zeros_like(st.err[..., 0]),
                paired.mse_of(st), paired.mae_of(st)]
        part = torch.stack(cols, -1).sum(1)                                   # (R, 4)
        if self.sums is not None and self.sums.shape != part.shape:
            raise ValueError(f"ContentPreservation.add: {part.shape[0]} rows after {self.sums.shape[0]}")
        self.sums = part if self.sums is None else self.sums + part
        self.count += batch.shape[0]
        self.data_range = st.data_range

    def result(self):
        if self.sums is None:
            raise RuntimeError("no batch has been added yet")
        m = (self.sums / self.count).cpu()
        return {"ssim": m[:, 0], "ms_ssim": m[:, 1] if self.ms else None, "mse": m[:, 2], "mae": m[:, 3],
                "psnr": 10.0 * torch.log10(self.data_range * self.data_range / m[:, 2]), "count": self.count}


class PerceptualDistance:
    """Is it still the same scene to a viewer, and does the condition do anything?  ``wu.lpips`` accumulated over a data set.
    ``add(batch, fakes)``: batch (B, 3, H, W), fakes (R, B, 3, H, W) as ``sweep`` returns them (R fixed across calls); sums kept in fp64 on the
    device, no host synchronisation.  ``result()``: ``lpips`` (R,) fp64 CPU, the per-row mean over all images of lpips(image, its output);
    ``diversity``, the mean over all images of the mean pairwise LPIPS among an image's R outputs (None with diversity=False or R = 1);
    and the image ``count``.  ``lpips_model`` is a ``wu.lpips.LPIPS`` with its weights loaded."""

    def __init__(self, lpips_model, value_range=(-1, 1), diversity=True, max_images=None):
        self.model, self.value_range, self.diversity = lpips_model, value_range, bool(diversity)
        self.max_images = max_images
        self.sums, self.div_sum, self.count = None, None, 0

    @torch.no_grad()
    def add(self, batch, fakes):
        from . import lpips
        if fakes.dim() != 5:
            raise ValueError(f"PerceptualDistance.add: fakes must be (R, B, 3, H, W), got {tuple(fakes.shape)}")
        mi = lpips.DEFAULT_MAX_IMAGES if self.max_images is None else self.max_images
        part = self.model.distance(batch, fakes, self.value_range, max_images=mi).sum(1)          # (R,)
        if self.sums is not None and self.sums.shape != part.shape:
            raise ValueError(f"PerceptualDistance.add: {part.shape[0]} rows after {self.sums.shape[0]}")
        self.sums = part if self.sums is None else self.sums + part
        if self.diversity and fakes.shape[0] >= 2:
            d = self.model.diversity(fakes, self.value_range, max_images=mi).sum()
            self.div_sum = d if self.div_sum is None else self.div_sum + d
        self.count += batch.shape[0]

    def result(self):
        if self.sums is None:
            raise RuntimeError("no batch has been added yet")
        return {"lpips": (self.sums / self.count).cpu(), "diversity": None if self.div_sum is None else (self.div_sum / self.count).item(),
                "count": self.count}


class SlicedWasserstein:
    """At which spatial scale do the outputs depart from the photographs?  ``wu.swd`` accumulated over a data set.  ``update(real, fake)``:
    real (B, 3, H, W), fake (B, 3, H, W) or (R, B, 3, H, W) as ``sweep`` returns it (R and the image size fixed across calls); the raw
    descriptors of the batch are gathered and kept on the device, 75 KB per image and level, no host synchronisation.  Image i of the
    stream gets the positions ``wu.swd.draw`` gives image i, so any split into batches equals one call on the concatenation, bit for bit.
    ``compute()`` normalises, projects, sorts and reports: a ``wu.swd.SWDResult`` (per-level values x 1e3, finest level first, and their
    mean), or a list of R of them when ``fake`` came with rows.
    ``reference``: a ``wu.swd.DescriptorBank``, or a list of R of them, one per row -- the photographs of the target class, say, of any
    count.  ``update`` then gathers only ``fake``, and ``compute()`` compares row r's outputs with ``reference[r]`` (or with the one bank)
    by the exact W1 for unequal counts (``wu.swd.compare`` of the row's outputs and that bank, bit for bit); a bank that serves several
    rows is normalised and sorted once per direction group, not once per row.  The banks must share this accumulator's P, seed, number
    of directions, levels, image size and value-range mapping (ValueError in ``compute``).  ``None``: as before."""

    def __init__(self, P=128, repeats=4, dirs_per_repeat=128, seed=0, value_range=(-1, 1), levels=None, dir_chunk=0, reference=None):
        self.P, self.ndirs, self.seed = int(P), int(repeats) * int(dirs_per_repeat), seed
        self.value_range, self.levels, self.dir_chunk = value_range, levels, int(dir_chunk)
        self.count, self.shape, self.rows = 0, None, None
        self.real, self.fake = [], []
        self.reference = list(reference) if isinstance(reference, (list, tuple)) else reference

    @torch.no_grad()
    def update(self, real, fake):
        from . import swd
        if not (torch.is_tensor(real) and torch.is_tensor(fake) and real.is_cuda and fake.is_cuda):
            raise RuntimeError("wu.evaluate.SlicedWasserstein: CUDA tensors only -- no CPU fallback")
        if real.dim() != 4 or fake.dim() not in (4, 5) or tuple(fake.shape[-4:]) != tuple(real.shape):
            raise ValueError(f"SlicedWasserstein.update: real (B, 3, H, W) and fake (B, 3, H, W) or (R, B, 3, H, W), got "
                             f"{tuple(real.shape)} / {tuple(fake.shape)}")
        b, _, h, w = real.shape
        rows = fake.shape[0] if fake.dim() == 5 else None
        if self.shape is None:
            self.shape, self.rows = (h, w), rows
            if self.levels is None:
                self.levels = swd.default_levels(h, w)
        elif self.shape != (h, w) or self.rows != rows:
            raise ValueError(f"SlicedWasserstein.update: {h} x {w} with rows {rows} after {self.shape[0]} x {self.shape[1]} with rows {self.rows}")
        shapes = swd.check_levels(h, w, self.levels)
        pos, _ = swd.draw(self.seed, self.levels, shapes, b, self.P, self.ndirs, first=self.count)
        if self.reference is None:
            self.real.append(swd.descriptors(real, pos, self.value_range, self.levels))
        self.fake.append([swd.descriptors(f, pos, self.value_range, self.levels) for f in (fake if rows is not None else fake[None])])
        self.count += b

    def compute(self):
        from . import swd
        if not self.fake:
            raise RuntimeError("no batch has been added yet")
        shapes = swd.check_levels(*self.shape, self.levels)
        _, dirs = swd.draw(self.seed, self.levels, shapes, 1, 1, self.ndirs)
        if self.reference is not None:
            return self._against_reference(dirs)
        real = [torch.cat([part[l] for part in self.real]) for l in range(self.levels)]
        out = []
        for r in range(len(self.fake[0])):
            fake = [torch.cat([part[r][l] for part in self.fake]) for l in range(self.levels)]
            out.append(swd.report(swd.distances(real, fake, dirs, self.dir_chunk).tolist()))
        return out if self.rows is not None else out[0]

    def _against_reference(self, dirs):
        from . import swd
        from .paired import range_mapping
        nrows = len(self.fake[0])
        banks = self.reference if isinstance(self.reference, list) else [self.reference] * nrows
        if len(banks) != nrows:
            raise ValueError(f"SlicedWasserstein: {len(banks)} reference banks for {nrows} rows")
        mine = {"P": self.P, "seed": self.seed, "ndirs": self.ndirs, "levels": self.levels, "image size": self.shape,
                "value-range mapping": tuple(range_mapping(self.value_range)[:2])}
        out = [None] * nrows
        for bank in {id(b): b for b in banks}.values():             # each distinct bank once, with all the rows it serves
            swd.check_comparable(mine, bank.signature(), "SlicedWasserstein(reference=)")
            rows = [r for r in range(nrows) if banks[r] is bank]
            fakes = [[torch.cat([part[r][l] for part in self.fake]) for l in range(self.levels)] for r in rows]
            for r, values in zip(rows, swd.distances_to_rows(bank.descriptors(), fakes, dirs, self.dir_chunk).tolist()):
                out[r] = swd.report(values)
        return out if self.rows is not None else out[0]


class SpectralDiscrepancy:
    """At which frequencies do the outputs depart from the photographs?  ``wu.spectrum`` accumulated over a data set.  ``update(real, fake)``:
    real (B, C, H, W), fake (B, C, H, W) or (R, B, C, H, W) as ``sweep`` returns it (R and the image size fixed across calls); each side's
    radial profiles go into a ``wu.spectrum.SpectrumBank`` (two sums per bin, fp64 on the device, no host synchronisation).  ``compute()``:
    a ``wu.spectrum.SpectrumResult`` (side a = the photographs, side b = the outputs), or a list of R of them when ``fake`` came with rows.
    ``reference``: a ``SpectrumBank``, or a list of R of them, one per row, used in place of ``real`` (``update`` then ignores ``real``);
    it must share this accumulator's image size, window and value-range mapping (ValueError in ``compute``)."""

    def __init__(self, value_range=(-1, 1), window="none", reference=None):
        from . import spectrum
        if window not in spectrum.WINDOWS:
            raise ValueError(f"SpectralDiscrepancy: window must be one of {spectrum.WINDOWS}, got {window!r}")
        self.value_range, self.window = value_range, window
        self.reference = list(reference) if isinstance(reference, (list, tuple)) else reference
        self.rows, self.real, self.fake = None, None, None

    @torch.no_grad()
    def update(self, real, fake):
        from . import spectrum
        if not (torch.is_tensor(real) and torch.is_tensor(fake) and real.is_cuda and fake.is_cuda):
            raise RuntimeError("wu.evaluate.SpectralDiscrepancy: CUDA tensors only -- no CPU fallback")
        if real.dim() != 4 or fake.dim() not in (4, 5) or tuple(fake.shape[-4:]) != tuple(real.shape):
            raise ValueError(f"SpectralDiscrepancy.update: real (B, C, H, W) and fake (B, C, H, W) or (R, B, C, H, W), got "
                             f"{tuple(real.shape)} / {tuple(fake.shape)}")
        rows = fake.shape[0] if fake.dim() == 5 else None
        if self.fake is None:
            self.rows = rows
            self.real = spectrum.SpectrumBank(self.value_range, self.window)
            self.fake = [spectrum.SpectrumBank(self.value_range, self.window) for _ in range(rows if rows is not None else 1)]
        elif self.rows != rows:
            raise ValueError(f"SpectralDiscrepancy.update: rows {rows} after rows {self.rows}")
        if self.reference is None:
            self.real.add(real)
        for bank, f in zip(self.fake, fake if rows is not None else fake[None]):
            bank.add(f)

    def compute(self):
        from . import spectrum
        if self.fake is None:
            raise RuntimeError("no batch has been added yet")
        nrows = len(self.fake)
        if self.reference is None:
            banks = [self.real] * nrows
        else:
            banks = self.reference if isinstance(self.reference, list) else [self.reference] * nrows
            if len(banks) != nrows:
                raise ValueError(f"SpectralDiscrepancy: {len(banks)} reference banks for {nrows} rows")
            for bank in banks:
                spectrum.check_comparable(self.fake[0].signature(), bank.signature(), "SpectralDiscrepancy(reference=)")
        out = [spectrum.compare(a, b) for a, b in zip(banks, self.fake)]
        return out if self.rows is not None else out[0]


class ClassTransferEval(_Confusion):
    """eval_class_transfer.py:106-136.  ``update(batch)`` transfers every image of the batch to every class (``transfer.sweep`` over the
    identity rows: the encoder runs once per batch), runs ``classifier`` over the nc * B outputs in passes of at most ``max_images`` images
    and counts arg-max of its fp32 logits (the script's Softmax does not move the arg-max) against the TARGET class.  The script's loop runs
    ``for i in range(bs)`` over ``onehot[i]``, i.e. it assumes batch size == number of classes; this one always covers all classes, like
    ``infer_driver.class_sweep``.  ``confusion()``: int64 (nc, nc), rows = target class, columns = predicted class; ``report()``:
    ``classification_report`` of it.  With the generator's dropout active the masks are those of ``sweep`` (the repeated-batch forward).
    ``content``: a ``ContentPreservation`` that also receives every (batch, sweep output), one row per class.
    ``swd``: a ``SlicedWasserstein`` that receives them too (``update(batch, fakes)``), one result per class.
    ``lpips``: a ``PerceptualDistance`` that receives them too (``add(batch, fakes)``), one row per class.
    ``spectrum``: a ``SpectralDiscrepancy`` that receives them too (``update(batch, fakes)``), one result per class."""

    def __init__(self, transfer, classifier, num_classes, max_images=SWEEP_MAX_IMAGES, names=None, content=None, swd=None, lpips=None,
                 spectrum=None):
        super().__init__(num_classes, names)
        self.transfer, self.classifier, self.max_images, self.content, self.swd = transfer, classifier, int(max_images), content, swd
        self.lpips, self.spectrum = lpips, spectrum

    @torch.no_grad()
    def update(self, batch):
        nc, b = self.num_classes, batch.shape[0]
        fakes = self.transfer.sweep(batch, torch.eye(nc, device=batch.device), self.max_images)
        logits = _batched(self.classifier, fakes.view(nc * b, *batch.shape[1:]), self.max_images)
        self.add(torch.arange(nc, device=batch.device).repeat_interleave(b), logits.argmax(1))
        if self.content is not None:
            self.content.add(batch, fakes)
        if self.swd is not None:
            self.swd.update(batch, fakes)
        if self.lpips is not None:
            self.lpips.add(batch, fakes)
        if self.spectrum is not None:
            self.spectrum.update(batch, fakes)


class EstimatorTransferEval(_Rows):
    """eval_estimator_transfer.py:48-61,129-130.  ``update(batch, ref_signals)`` transfers every image of the batch to every row of
    ``ref_signals`` (R, nc) (``transfer.sweep``), runs ``estimator`` over the outputs and appends, per row, the batch mean of
    ``pred - row`` (:54-57); ``result()``: fp64 ``mean`` and population ``std`` over all appended rows (:129-130) and their ``count``.
    ``content``: a ``ContentPreservation`` that also receives every (batch, sweep output), one row per reference row.
    ``swd``: a ``SlicedWasserstein`` that receives them too (``update(batch, fakes)``), one result per reference row.
    ``lpips``: a ``PerceptualDistance`` that receives them too (``add(batch, fakes)``), one row per reference row.
    ``spectrum``: a ``SpectralDiscrepancy`` that receives them too (``update(batch, fakes)``), one result per reference row."""

    def __init__(self, transfer, estimator, max_images=SWEEP_MAX_IMAGES, content=None, swd=None, lpips=None, spectrum=None):
        super().__init__()
        self.transfer, self.estimator, self.max_images, self.content, self.swd = transfer, estimator, int(max_images), content, swd
        self.lpips, self.spectrum = lpips, spectrum

    @torch.no_grad()
    def update(self, batch, ref_signals):
        ref = ref_signals.to(device=batch.device, dtype=torch.float32)
        r, b = ref.shape[0], batch.shape[0]
        fakes = self.transfer.sweep(batch, ref, self.max_images)
        pred = _batched(self.estimator, fakes.view(r * b, *batch.shape[1:]), self.max_images).view(r, b, -1)
        self.add((pred - ref.unsqueeze(1)).mean(1))
        if self.content is not None:
            self.content.add(batch, fakes)
        if self.swd is not None:
            self.swd.update(batch, fakes)
        if self.lpips is not None:
            self.lpips.add(batch, fakes)
        if self.spectrum is not None:
            self.spectrum.update(batch, fakes)


class ClassifierEval(_Confusion):
    """eval_classifier_i2w.py:85-106: the classifier on the photographs themselves.  ``update(batch, labels)`` counts arg-max of the fp32
    logits against the class indices ``labels``; rows of the matrix = true class, columns = predicted class."""

    def __init__(self, classifier, num_classes, names=None):
        super().__init__(num_classes, names)
        self.classifier = classifier

    @torch.no_grad()
    def update(self, batch, labels):
        self.add(labels.to(batch.device), self.classifier(batch).float().argmax(1))


class EstimatorEval(_Rows):
    """eval_estimator.py:141-159: the estimator on the photographs themselves.  ``update(batch, signals)`` appends ``pred - signals``
    (one row per image); ``result()``: fp64 ``mean`` / population ``std`` of those errors and ``mse``, the mean squared error per signal."""

    def __init__(self, estimator):
        super().__init__()
        self.estimator = estimator

    @torch.no_grad()
    def update(self, batch, signals):
        self.add(self.estimator(batch).float() - signals.to(device=batch.device, dtype=torch.float32))

    def result(self):
        return super().result(mse=True)
