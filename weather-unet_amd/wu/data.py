"""File -> JPEG decoder -> input pipeline, batch by batch: replaces the reference's ``DataLoader`` + torchvision transforms
(dataset.py:56-150 with t_cls_train.py:81-125; the class-balancing sampler of sampler.py).

    loader = JpegBatchLoader(paths, labels, batch_size=32, pipeline=GPUInputPipeline(224, augmentation=True, seed=0),
                             sample_weights=class_balanced_weights(labels), seed=0, drop_last=True)
    for images, targets, batch_paths in loader:         # images (N, 3, S, S) fp32 CUDA in [-1, 1]
        ...

A background thread runs ``decoder.prepare`` (file read + Huffman decoding on the decoder's thread pool) up to ``prefetch`` batches
ahead; ``decoder.finish`` and the pipeline run in the consumer's thread, on its current stream.  The order of samples is a pure
function of (len(paths), shuffle, sample_weights, num_samples, seed, epoch).
"""
import queue
import random
import threading

import numpy as np
import torch


def class_balanced_weights(labels):
    """1 / count[label] per sample: the weights of the reference's ImbalancedDatasetSampler (sampler.py:28-39)."""
    labels = [x.item() if hasattr(x, "item") else x for x in labels]
    count = {}
    for x in labels:
        count[x] = count.get(x, 0) + 1
    return [1.0 / count[x] for x in labels]


class JpegBatchLoader:
    """Iterable over ``(images | (src_u8, sizes) when pipeline is None, targets tensor or None, paths)``.

    shuffle: a seeded permutation per epoch.  sample_weights: ``num_samples`` (default len(paths)) indices drawn with replacement per
    epoch by ``torch.multinomial`` from a seeded generator (sampler.py:52-54).  Every ``__iter__`` is one epoch; the epoch counter
    advances the seed.  Leaving an epoch early (break, exception, ``close()``) stops and joins its background thread."""

    def __init__(self, paths, targets=None, batch_size=16, pipeline=None, decoder=None, shuffle=False, sample_weights=None,
                 num_samples=None, seed=None, drop_last=False, prefetch=2, png_decode=False, jpeg_coverage="baseline"):
        self.paths = list(paths)
        if not self.paths:
            raise ValueError("JpegBatchLoader: no files")
        if targets is not None and len(targets) != len(self.paths):
            raise ValueError("JpegBatchLoader: one target per file")
        if sample_weights is not None and len(sample_weights) != len(self.paths):
            raise ValueError("JpegBatchLoader: one weight per file")
        if batch_size < 1 or prefetch < 1:
            raise ValueError("JpegBatchLoader: batch_size and prefetch must be >= 1")
        self.targets = targets
        self.batch_size, self.pipeline, self.shuffle, self.drop_last, self.prefetch = int(batch_size), pipeline, bool(shuffle), bool(drop_last), int(prefetch)
        self.weights = None if sample_weights is None else torch.as_tensor(np.asarray(sample_weights, dtype=np.float64))
        self.num_samples = len(self.paths) if num_samples is None else int(num_samples)
        self.seed = random.SystemRandom().randrange(2 ** 31) if seed is None else int(seed)
        if decoder is None and png_decode:                # opt-in: a directory of segmented PNGs (wu.png_enc's) inflated on the GPU
            from .png import GPUPngDecoder
            decoder = GPUPngDecoder()
        if decoder is None:
            from .jpeg import GPUJpegDecoder
            decoder = GPUJpegDecoder(coverage=jpeg_coverage)          # "extended": progressive and 4:4:0 files natively too (opt-in)
        self.decoder = decoder
        self.epoch = 0
        self._active = []
        self._lock = threading.Lock()

    # ---- order ----
    def epoch_indices(self, epoch):
        g = torch.Generator()
        g.manual_seed(self.seed + int(epoch))
        if self.weights is not None:
            return torch.multinomial(self.weights, self.num_samples, replacement=True, generator=g).tolist()
        if self.shuffle:
            return torch.randperm(len(self.paths), generator=g).tolist()
        return list(range(len(self.paths)))

    def epoch_batches(self, epoch):
        idx = self.epoch_indices(epoch)
        out = [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]
        if self.drop_last and out and len(out[-1]) < self.batch_size:
            out.pop()
        return out

    def __len__(self):
        n = self.num_samples if self.weights is not None else len(self.paths)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    # ---- iteration ----
    def __iter__(self):
        ep = _Epoch(self, self.epoch_batches(self.epoch))
        self.epoch += 1
        with self._lock:
            self._active.append(ep)
        return ep.run()

    def _done(self, ep):
        with self._lock:
            if ep in self._active:
                self._active.remove(ep)

    def close(self):
        """Stop and join the background thread of every epoch still in flight."""
        with self._lock:
            active = list(self._active)
        for ep in active:
            ep.stop()

    def _targets_of(self, idx, like):
        if self.targets is None:
            return None
        t = torch.as_tensor(np.stack([np.asarray(self.targets[i]) for i in idx]))
        return t.to(like.device, non_blocking=True) if torch.is_tensor(like) and like.is_cuda else t


class _Epoch:
    def __init__(self, loader, batches):
        self.loader, self.batches = loader, batches
        self.q = queue.Queue(maxsize=loader.prefetch)
        self.halt = threading.Event()
        self.thread = threading.Thread(target=self._produce, name="wu-jpeg-loader", daemon=True)
        self.thread.start()

    def _put(self, item):
        while not self.halt.is_set():
            try:
                self.q.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _produce(self):
        try:
            for idx in self.batches:
                if self.halt.is_set():
                    return
                paths = [self.loader.paths[i] for i in idx]
                hb = self.loader.decoder.prepare(paths)
                if not self._put((idx, paths, hb)):
                    _release(hb)
                    return
            self._put(None)
        except BaseException as e:            # noqa: BLE001 -- handed to the consumer, which re-raises it
            self._put(e)

    def stop(self):
        self.halt.set()
        while self.thread.is_alive():
            self._drain()
            self.thread.join(timeout=0.05)
        self._drain()
        self.loader._done(self)

    def _drain(self):
        try:
            while True:
                item = self.q.get_nowait()
                if isinstance(item, tuple):
                    _release(item[2])
        except queue.Empty:
            pass

    def run(self):
        ld = self.loader
        try:
            while True:
                item = self.q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                idx, paths, hb = item
                try:
                    src_u8, sizes = ld.decoder.finish(hb)
                finally:
                    _release(hb)
                images = ld.pipeline(src_u8, sizes) if ld.pipeline is not None else (src_u8, sizes)
                yield images, ld._targets_of(idx, src_u8), paths
        finally:
            self.stop()


def _release(hb):
    rel = getattr(hb, "release", None)
    if rel is not None:
        rel()
