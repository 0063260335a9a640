"""FID and Inception Score on the HIP InceptionV3 (the reference's eval/fid_score.py and eval/inception_score.py).

    python -m wu.fid PATH1 PATH2 --weights pt_inception-2015-12-05-6726825d.pth [--dims 2048] [--batch-size 50] [--precision fp32|bf16]

Each PATH is a directory of ``.jpg`` / ``.png`` images of one size or a ``.npz`` file with ``mu`` / ``sigma`` (fid_score.py's format, in
both directions: ``FIDStatistics.save_npz`` writes it).  The weight file is the user's (pytorch-fid's FID Inception weights); nothing is
downloaded.

Feature statistics never leave the GPU per batch: ``FIDStatistics.update`` runs the network and adds the batch's shifted first and second
moments into fp64 device accumulators (wu_feature_stats_update); ``finalize`` turns them into ``mu`` and the unbiased ``sigma``
(np.cov(rowvar=False)).  The Frechet distance itself (a matrix square root of a D x D product) runs on the host in float64 with scipy.

``--kid`` adds the Kernel Inception Distance (wu.kid: the unbiased polynomial-kernel MMD^2 over random subsets of the same feature rows,
on the fp64 matrix cores), the metric to read on a few hundred images, where the covariance above is rank-deficient.  It needs the rows
themselves: a ``.npz`` PATH must then hold ``features`` (``wu.features.FeatureBank.save_npz``); ``mu`` / ``sigma`` are computed from the rows
when the file lacks them.

``--fid-rows`` adds the rank-aware Frechet distance of the same rows (wu.frechet: Tr sqrt(sigma1 sigma2) as the nuclear norm of the centred
cross-Gram matrix, by a Jacobi iteration on the GPU), printed as ``FID (rows): <value> (<sweeps> sweeps)`` after the FID line: no 2048 x 2048
covariance and no sqrtm, so it is exact on a few hundred images.  It needs ``features`` in a ``.npz`` PATH just as ``--kid`` does.

``--prdc`` adds improved precision / recall and density / coverage (wu.prdc: k-NN manifold membership on the same rows, PATH1 the real
set), which tell a loss of diversity from a loss of fidelity; it needs ``features`` in a ``.npz`` PATH just as ``--kid`` does.

``--nn K`` adds one ``NN:`` line on the rows of PATH2 against the bank of PATH1 (wu.retrieval: each row's K nearest rows of PATH1): the
median and the smallest nearest distance and, with ``--nn-threshold T``, how many rows lie closer than T to a row of PATH1 -- copies of
training photographs among generated images, or test photographs whose near-duplicate sits in the training set.  ``--nn-report`` writes
the per-row answer as JSON.  It needs ``features`` in a ``.npz`` PATH just as ``--kid`` does.

``--resize clean`` brings the images to 299 x 299 with Pillow's antialiased bicubic filter on float32 channels, without quantisation
(wu.resample, float mode; Parmar et al., CVPR 2022), instead of the aliased bilinear interpolation of pytorch-fid (``legacy``, the default),
and reads directories of MIXED image sizes.  It is the resize rule only: network and weights stay pytorch-fid's, so the numbers are not
comparable with the statistics files the ``clean-fid`` package publishes.  ``.npz`` files record the rule they were computed under (no key:
legacy); paths under different rules raise.
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import _lib
from .features import FeatureBank, as_rows
from .files import image_files, pass_decoder, read_batches, same_size
from .inception import InceptionV3, global_avgpool
from .layout import precision_code, stream_ptr

LEGACY, CLEAN = "legacy", "clean"         # the resize rules of InceptionV3(resize=...)


class FIDStatistics:
    """Running mean / covariance of InceptionV3 features (the first requested block of ``model``: pool3 by default).

    ``update(images, value_range=(0, 1))``: (N, 3, H, W) float32 in ``value_range`` or (N, H, W, 3) uint8 on the GPU.  Spatial blocks
    (dims 64 / 192 / 768) are averaged over H x W first, as fid_score.py's adaptive_avg_pool2d does."""

    def __init__(self, model):
        self.model = model
        self.n = 0
        self._sum = self._cross = self._shift = None

    def update(self, images, value_range=(0, 1), features=None, sizes=None):
        """``features``: a wu.features.FeatureBank that also receives the batch's rows (for the KID).  ``sizes``: [(h, w)] per image of a
        padded ragged uint8 batch (a model with ``resize="clean"`` only)."""
        feat = self.model(images, value_range=value_range)[0] if sizes is None else self.model(images, value_range=value_range, sizes=sizes)[0]
        n, c, h, w = feat.shape
        if h * w != 1 or feat.dtype != torch.float32:
            feat = global_avgpool(feat, precision_code(self.model.precision))
        else:
            feat = feat.permute(0, 2, 3, 1).reshape(n, c)          # the (N, 1, 1, C) buffer itself
        self.update_features(feat)
        if features is not None:
            features.append(feat)

    def update_features(self, feats):
        """Add a batch of feature rows (B, D) float32 on the GPU."""
        feats = as_rows(feats, "FIDStatistics.update_features")
        b, d = feats.shape
        first = self._sum is None
        if first:
            self._sum = torch.zeros(d, dtype=torch.float64, device=feats.device)
            self._cross = torch.zeros(d, d, dtype=torch.float64, device=feats.device)
            self._shift = torch.zeros(d, dtype=torch.float32, device=feats.device)
        elif d != self._sum.numel():
            raise ValueError(f"FIDStatistics: feature width {d} differs from the first batch's {self._sum.numel()}")
        _lib.call("wu_feature_stats_update", feats.data_ptr(), feats.stride(0), b, d, self._shift.data_ptr(), 1 if first else 0,
                  self._sum.data_ptr(), self._cross.data_ptr(), stream_ptr())
        self.n += b

    def finalize(self):
        """(mu, sigma) float64 numpy: the sample mean and the unbiased sample covariance of every row seen."""
        if self.n < 2:
            raise ValueError(f"FIDStatistics: need at least 2 feature rows, have {self.n}")
        k = self._shift.double().cpu().numpy()
        s = self._sum.cpu().numpy()
        cross = self._cross.cpu().numpy()
        m = s / self.n
        mu = k + m
        sigma = (cross - self.n * np.outer(m, m)) / (self.n - 1)
        return mu, sigma

    def save_npz(self, path):
        """``mu`` / ``sigma``, and the resize rule under ``resize`` when it is not the legacy one (a file without the key is legacy)."""
        mu, sigma = self.finalize()
        rule = getattr(self.model, "resize", LEGACY)
        np.savez(path, mu=mu, sigma=sigma, **({} if rule == LEGACY else {"resize": np.array(rule)}))


def npz_resize_rule(path):
    """The resize rule a statistics / feature file was recorded under: its ``resize`` key, ``"legacy"`` without one."""
    with np.load(path) as f:
        return str(f["resize"]) if "resize" in f else LEGACY


def check_same_resize(paths, resize):
    """Raise if the paths were (or would be) evaluated under different resize rules: a directory under ``resize``, a .npz under the
    rule it records.  Statistics under the aliased and under the antialiased resize differ by more than models do."""
    rules = [npz_resize_rule(p) if p.endswith(".npz") else resize for p in paths]
    if len(set(rules)) > 1:
        raise ValueError("resize rules differ: " + ", ".join(f"{p}: {r}" for p, r in zip(paths, rules)) +
                         " (statistics recorded under different resize rules are not comparable)")


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = ||mu1 - mu2||^2 + Tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)), float64 (fid_score.py's semantics: scipy's sqrtm of the
    product; the eps * I offset retry when it is not finite; a ValueError when the imaginary part of the diagonal exceeds 1e-3)."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def inception_score(logits_or_probs, splits=1, is_logits=None):
    """exp(mean_x KL(p(y|x) || p(y))) per split of the N rows; returns (mean, std) over the splits (inception_score.py).
    ``is_logits``: None = probabilities if every row is non-negative and sums to 1 (to 1e-3), else logits (softmax in float64)."""
    a = logits_or_probs.detach().cpu().double().numpy() if torch.is_tensor(logits_or_probs) else np.asarray(logits_or_probs, dtype=np.float64)
    if is_logits is None:
        is_logits = not (np.all(a >= 0) and np.allclose(a.sum(axis=1), 1.0, atol=1e-3))
    if is_logits:
        e = np.exp(a - a.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    else:
        p = a / a.sum(axis=1, keepdims=True)           # scipy.stats.entropy normalises its arguments
    n = p.shape[0]
    scores = []
    for k in range(splits):
        part = p[k * (n // splits):(k + 1) * (n // splits)]
        py = part.mean(axis=0)
        py = py / py.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = np.where(part > 0, part * np.log(part / py), 0.0).sum(axis=1)
        scores.append(np.exp(kl.mean()))
    return float(np.mean(scores)), float(np.std(scores))


# ----------------------------------------------------------------------------------------------
# command line (fid_score.py)
# ----------------------------------------------------------------------------------------------
def statistics_of_path(path, model, batch_size, gpu_decode=False, gpu_decode_png=False, gpu_entropy=False, features=None, resize=None,
                       gpu_extended=False):
    """(mu, sigma) of a .npz file or of the images in a directory (uint8 batches straight to the GPU).  gpu_decode: read the files
    through wu.jpeg.GPUJpegDecoder instead of the per-file Pillow loop; gpu_decode_png: through wu.png.GPUPngDecoder, which inflates the
    segmented PNGs wu.png_enc writes on the GPU and hands every other file to Pillow -- the same uint8 batch, hence the same statistics.
    gpu_entropy (implies gpu_decode): the JPEG decoder also Huffman-decodes on the GPU (``entropy="device"``).  gpu_extended (implies
    gpu_decode): the JPEG decoder reads progressive and 4:4:0 files natively too (``coverage="extended"``).  All off by default.
    features: a wu.features.FeatureBank that also receives every feature row (the KID's input); a .npz must then hold ``features``, and its
    ``mu`` / ``sigma`` are taken from the file when it has them and computed from the rows when it does not.
    resize: the model's rule (``InceptionV3(resize=...)``; None: whatever the model has).  ``"clean"`` reads a directory of MIXED sizes on
    all three read paths, as the padded ragged batches of wu.files; ``"legacy"`` raises on a batch of mixed sizes, as it always has.
    A .npz recorded under another rule than ``resize`` raises."""
    if path.endswith(".npz"):
        if resize is not None and npz_resize_rule(path) != resize:
            raise ValueError(f"resize rules differ: {path} was recorded under {npz_resize_rule(path)!r}, not {resize!r}")
        if features is None:
            with np.load(path) as f:
                return f["mu"][:], f["sigma"][:]
        return _npz_statistics_and_features(path, features)
    rule = getattr(model, "resize", LEGACY)
    if resize is not None and resize != rule:
        raise ValueError(f"statistics_of_path: resize={resize!r}, but the model was built with resize={rule!r}")
    files = image_files(path)
    if not files:
        raise RuntimeError(f"no .jpg / .png images in {path}")
    stats = FIDStatistics(model)
    if features is not None and rule != LEGACY:
        features.resize = rule
    with pass_decoder(gpu_decode, gpu_decode_png, gpu_entropy, gpu_extended) as dec:
        for batch, sizes in read_batches(files, batch_size, dec):
            if rule == CLEAN:
                stats.update(batch, features=features, sizes=sizes)
            else:
                same_size(sizes, f"in {path}: ")          # per batch, as pytorch-fid's np.stack refuses
                stats.update(batch, features=features)
    return stats.finalize()


def _npz_statistics_and_features(path, features):
    bank = FeatureBank.load_npz(path)
    features.resize = bank.resize
    if bank.n:
        features.append(bank.features)
    with np.load(path) as f:
        if "mu" in f and "sigma" in f:
            return f["mu"][:], f["sigma"][:]
    stats = FIDStatistics(None)
    stats.update_features(bank.features)
    return stats.finalize()


def _pass_over_paths(paths, weights, batch_size, dims, precision, gpu_decode=False, gpu_decode_png=False, gpu_entropy=False, *, fid, rows,
                     resize=LEGACY, gpu_extended=False):
    """What every entry point below shares: the path check, the model loaded once (not at all for .npz files alone) and ONE pass over each
    path.  Returns (stats, banks), a list per path each: (mu, sigma) when ``fid`` and a FeatureBank of the feature rows when ``rows``, None
    otherwise.  Without ``rows`` a .npz is read for ``mu`` / ``sigma`` only; with ``rows`` it must hold ``features``, and without ``fid``
    it needs nothing else.  ``resize``: the rule directories are read under (``InceptionV3(resize=...)``); paths under different rules --
    a .npz records its own -- raise before anything is computed."""
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError(f"Invalid path: {p}")
    if resize not in (LEGACY, CLEAN):
        raise ValueError(f"resize must be {LEGACY!r} or {CLEAN!r}, got {resize!r}")
    check_same_resize(paths, resize)
    model = None
    if not all(p.endswith(".npz") for p in paths):
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]], precision=precision, resize=resize)
        model.load_state_dict(torch.load(weights, map_location="cpu"))
    stats, banks = [], []
    for p in paths:
        bank = FeatureBank() if rows else None
        if rows and not fid and p.endswith(".npz"):
            loaded = FeatureBank.load_npz(p)
            bank.append(loaded.features)
            bank.resize = loaded.resize
            st = None
        else:
            st = statistics_of_path(p, model, batch_size, gpu_decode, gpu_decode_png, gpu_entropy, features=bank,
                                    resize=None if p.endswith(".npz") else resize,      # a .npz keeps its own rule (checked above)
                                    gpu_extended=gpu_extended)
        stats.append(st if fid else None)
        banks.append(bank)
    return stats, banks


def calculate_fid_given_paths(paths, weights, batch_size=50, dims=2048, precision="fp32", gpu_decode=False, gpu_decode_png=False,
                              gpu_entropy=False, resize=LEGACY):
    stats, _ = _pass_over_paths(paths, weights, batch_size, dims, precision, gpu_decode, gpu_decode_png, gpu_entropy, fid=True, rows=False,
                                resize=resize)
    return calculate_frechet_distance(*stats[0], *stats[1])


def calculate_fid_and_banks_given_paths(paths, weights, batch_size=50, dims=2048, precision="fp32", gpu_decode=False, gpu_decode_png=False,
                                        gpu_entropy=False, resize=LEGACY):
    """(fid, (bank1, bank2)) from ONE pass over each path: the feature rows feed the moment accumulators and a FeatureBank each, which
    wu.kid.kernel_inception_distance and wu.prdc.precision_recall_density_coverage then share (``--kid`` / ``--prdc``)."""
    stats, banks = _pass_over_paths(paths, weights, batch_size, dims, precision, gpu_decode, gpu_decode_png, gpu_entropy, fid=True, rows=True,
                                    resize=resize)
    return calculate_frechet_distance(*stats[0], *stats[1]), tuple(banks)


def calculate_fid_and_kid_given_paths(paths, weights, batch_size=50, dims=2048, precision="fp32", gpu_decode=False, gpu_decode_png=False,
                                      gpu_entropy=False, num_subsets=100, subset_size=1000, seed=2020, resize=LEGACY):
    """(fid, (kid_mean, kid_std)) from ONE pass over each path."""
    from .kid import kernel_inception_distance
    fid, banks = calculate_fid_and_banks_given_paths(paths, weights, batch_size, dims, precision, gpu_decode, gpu_decode_png, gpu_entropy,
                                                     resize=resize)
    return fid, kernel_inception_distance(*banks, num_subsets=num_subsets, subset_size=subset_size, seed=seed)


def calculate_kid_given_paths(paths, weights, batch_size=50, dims=2048, precision="fp32", gpu_decode=False, gpu_decode_png=False,
                              gpu_entropy=False, num_subsets=100, subset_size=1000, seed=2020, resize=LEGACY):
    """(mean, std) of the Kernel Inception Distance between two image directories / .npz files holding ``features``."""
    from .kid import kernel_inception_distance
    _, banks = _pass_over_paths(paths, weights, batch_size, dims, precision, gpu_decode, gpu_decode_png, gpu_entropy, fid=False, rows=True,
                                resize=resize)
    return kernel_inception_distance(*banks, num_subsets=num_subsets, subset_size=subset_size, seed=seed)


def calculate_prdc_given_paths(paths, weights, batch_size=50, dims=2048, precision="fp32", gpu_decode=False, gpu_decode_png=False,
                               gpu_entropy=False, k=5, resize=LEGACY):
    """wu.prdc.PRDC(precision, recall, density, coverage) of paths[1] (the generated set) against paths[0] (the real set): two image
    directories / .npz files holding ``features``, one pass over each."""
    from .prdc import precision_recall_density_coverage
    _, banks = _pass_over_paths(paths, weights, batch_size, dims, precision, gpu_decode, gpu_decode_png, gpu_entropy, fid=False, rows=True,
                                resize=resize)
    return precision_recall_density_coverage(*banks, k=k)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m wu.fid", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                 description="Frechet Inception Distance between two image directories / .npz statistics files")
    ap.add_argument("path", type=str, nargs=2, help="directories of images or .npz statistics files")
    ap.add_argument("--weights", required=True, help="pytorch-fid FID Inception weights (pt_inception-2015-12-05-*.pth)")
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--dims", type=int, default=2048, choices=list(InceptionV3.BLOCK_INDEX_BY_DIM))
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--gpu-decode", action="store_true", help="decode the image files with wu.jpeg.GPUJpegDecoder (HIP kernels) instead of Pillow")
    ap.add_argument("--gpu-entropy", action="store_true",
                    help="with --gpu-decode (implied): Huffman-decode the JPEG scans on the GPU too, so that the compressed scan and not the "
                         "coefficients goes over the link")
    ap.add_argument("--gpu-decode-extended", action="store_true",
                    help="with --gpu-decode (implied): decode progressive and 4:4:0 JPEG files natively too (coverage='extended'; the scans "
                         "of a progressive file are run on the host threads) instead of handing them to Pillow; not with --gpu-entropy")
    ap.add_argument("--gpu-decode-png", action="store_true",
                    help="decode segmented PNG files (what wu.png_enc writes) with wu.png.GPUPngDecoder (HIP kernels); other files go to Pillow")
    ap.add_argument("--resize", default=LEGACY, choices=[LEGACY, CLEAN],
                    help="how images reach 299 x 299: 'legacy' is pytorch-fid's bilinear interpolation without antialiasing; 'clean' is "
                         "Pillow's antialiased bicubic filter on float32 channels without quantisation (wu.resample; Parmar et al. 2022), "
                         "which also reads directories of mixed image sizes.  The rule only: network and weights stay pytorch-fid's, so the "
                         "numbers are not comparable with the statistics files the clean-fid package publishes")
    ap.add_argument("--kid", action="store_true",
                    help="also print the Kernel Inception Distance (mean and standard deviation over random subsets of the feature rows); "
                         "a .npz path must then hold 'features'")
    ap.add_argument("--kid-subsets", type=int, default=100, help="with --kid: number of subsets")
    ap.add_argument("--kid-subset-size", type=int, default=1000,
                    help="with --kid: rows per subset; an error, never clamped, when either path has fewer images")
    ap.add_argument("--kid-seed", type=int, default=2020, help="with --kid: seed of the subset draw (numpy RandomState)")
    ap.add_argument("--fid-rows", action="store_true",
                    help="also print the rank-aware Frechet distance computed from the feature rows on the GPU (wu.frechet: singular values "
                         "of the centred cross-Gram matrix, exact where the covariances are rank-deficient) and its Jacobi sweep count; a "
                         ".npz path must then hold 'features'")
    ap.add_argument("--prdc", action="store_true",
                    help="also print improved precision / recall and density / coverage of the second path against the first (the real "
                         "set); a .npz path must then hold 'features'")
    ap.add_argument("--prdc-k", type=int, default=5, help="with --prdc: the k of the k-NN radii (prdc's default 5; Kynkaanniemi et al. use 3)")
    ap.add_argument("--nn", type=int, default=0, metavar="K",
                    help="also print, for the rows of the second path, the distance to their nearest rows of the first (wu.retrieval: the "
                         "K nearest, 1..16; the line gives the median and the smallest nearest distance: leakage and memorisation); a "
                         ".npz path must then hold 'features'")
    ap.add_argument("--nn-threshold", type=float, default=None, metavar="T", help="with --nn: also count the rows closer than T to a row of the first path")
    ap.add_argument("--nn-report", default=None, metavar="OUT.json",
                    help="with --nn: write wu.retrieval.nearest_report's dict here; with --nn-radius it gains the full pair list (key 'radius_join')")
    ap.add_argument("--nn-radius", type=float, default=None, metavar="R",
                    help="also print, for the rows of the second path, EVERY row of the first within the distance R (wu.retrieval.radius_join: "
                         "pairs, rows with a hit, the most pairs of one row); a .npz path must then hold 'features'")
    ap.add_argument("--realism", action="store_true",
                    help="also print the per-row realism (Kynkaanniemi et al. 2019) and rarity (Han et al. 2022) summary of the rows of the "
                         "second path against the k-NN manifold of the first (wu.retrieval.ball_scores); a .npz path must then hold 'features'")
    ap.add_argument("--realism-k", type=int, default=3, help="with --realism: the k of the k-NN radii")
    ap.add_argument("--realism-report", default=None, metavar="OUT.json", help="with --realism: write wu.retrieval.score_report's dict here")
    args = ap.parse_args(argv)
    stats, banks = _pass_over_paths(args.path, args.weights, args.batch_size, args.dims, args.precision, args.gpu_decode, args.gpu_decode_png,
                                    args.gpu_entropy, fid=True, rows=args.kid or args.prdc or args.fid_rows or args.nn != 0 or args.nn_radius is not None
                                    or args.realism, resize=args.resize, gpu_extended=args.gpu_decode_extended)
    print(f"FID: {calculate_frechet_distance(*stats[0], *stats[1])}")
    if args.fid_rows:
        from .frechet import frechet_distance
        r = frechet_distance(*banks)
        print(f"FID (rows): {r.fid} ({r.sweeps} sweeps)")
    if args.kid:
        from .kid import kernel_inception_distance
        kid_mean, kid_std = kernel_inception_distance(*banks, num_subsets=args.kid_subsets, subset_size=args.kid_subset_size, seed=args.kid_seed)
        print(f"KID: {kid_mean} \u00b1 {kid_std}")
    if args.prdc:
        from .prdc import precision_recall_density_coverage
        m = precision_recall_density_coverage(*banks, k=args.prdc_k)
        print(f"PRDC: precision {m.precision} recall {m.recall} density {m.density} coverage {m.coverage}")
    if args.nn or args.nn_radius is not None or args.realism:
        import json
        from . import retrieval
        names = [None if p.endswith(".npz") else [f.name for f in image_files(p)] for p in args.path]
        rep = {}
        if args.nn:
            rep = retrieval.nearest_report(banks[1], banks[0], threshold=args.nn_threshold, query_names=names[1], bank_names=names[0], k=args.nn)
            print(retrieval.nn_line(rep))
        if args.nn_radius is not None:
            join = retrieval.radius_join(banks[1], banks[0], args.nn_radius * args.nn_radius)
            rep["radius_join"] = retrieval.radius_report(*join, args.nn_radius, names[1], names[0])
            print(retrieval.radius_line(rep["radius_join"]))
        if args.nn_report and rep:
            with open(args.nn_report, "w") as fh:
                json.dump(rep, fh)
        if args.realism:
            scores = retrieval.ball_scores(banks[1], banks[0], k=args.realism_k)
            srep = retrieval.score_report(scores, k=args.realism_k, query_names=names[1], bank_names=names[0])
            print(retrieval.realism_line(srep))
            if args.realism_report:
                with open(args.realism_report, "w") as fh:
                    json.dump(srep, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main())
