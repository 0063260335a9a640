"""CPU: the host side of the condition sweep and of wu/evaluate.py -- the classification report's arithmetic, the accumulators, the sweep's
chunking and seed draws, and the argument checks of the two new ABI functions (no compute is launched here)."""
import numpy as np
import pytest
import torch

# rows = true class, columns = predicted class; class 2 is never predicted (its precision is undefined -> 0)
CM = [[3, 1, 0],
      [1, 2, 0],
      [2, 1, 0]]
EXPECTED = {
    "0": {"precision": 3 / 6, "recall": 3 / 4, "f1-score": 0.6, "support": 4},
    "1": {"precision": 2 / 4, "recall": 2 / 3, "f1-score": 4 / 7, "support": 3},
    "2": {"precision": 0.0, "recall": 0.0, "f1-score": 0.0, "support": 3},
    "accuracy": 5 / 10,
    "macro avg": {"precision": (0.5 + 0.5 + 0) / 3, "recall": (3 / 4 + 2 / 3 + 0) / 3, "f1-score": (0.6 + 4 / 7 + 0) / 3, "support": 10},
    "weighted avg": {"precision": (4 * 0.5 + 3 * 0.5) / 10, "recall": (4 * 3 / 4 + 3 * 2 / 3) / 10, "f1-score": (4 * 0.6 + 3 * 4 / 7) / 10,
                     "support": 10},
}


def _assert_report(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        if isinstance(v, dict):
            assert sorted(got[k]) == sorted(v)
            for kk, vv in v.items():
                assert got[k][kk] == pytest.approx(vv, rel=1e-12, abs=1e-15), (k, kk)
        else:
            assert got[k] == pytest.approx(v, rel=1e-12), k


def test_report_on_a_hand_written_confusion_matrix():
    from wu.evaluate import classification_report
    _assert_report(classification_report(CM), EXPECTED)
    named = classification_report(torch.tensor(CM), names=["sunny", "cloudy", "rain"])
    assert named["rain"] == EXPECTED["2"] and "2" not in named
    # a class that occurs neither as truth nor as prediction is left out of the list and of the averages, as sklearn leaves it out
    wide = [r + [0] for r in CM] + [[0, 0, 0, 0]]
    _assert_report(classification_report(wide), EXPECTED)


def test_report_and_confusion_match_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from wu.evaluate import ClassifierEval, classification_report
    y_true, y_pred = [], []
    for t, row in enumerate(CM):
        for p, cnt in enumerate(row):
            y_true += [t] * cnt
            y_pred += [p] * cnt
    assert np.array_equal(metrics.confusion_matrix(y_true, y_pred, labels=np.arange(3)), np.array(CM))
    want = metrics.classification_report(y_true, y_pred, output_dict=True, zero_division=0)
    _assert_report(classification_report(CM), want)
    # the accumulator, fed in two batches through a "classifier" that returns one-hot logits of the wanted predictions
    ev = ClassifierEval(lambda batch: torch.eye(3)[batch.long().view(-1)], 3)
    yt, yp = torch.tensor(y_true), torch.tensor(y_pred)
    ev.update(yp[:4].float(), yt[:4])
    ev.update(yp[4:].float(), yt[4:])
    assert ev.confusion().dtype == torch.int64 and np.array_equal(ev.confusion().numpy(), np.array(CM))
    _assert_report(ev.report(), want)


def test_estimator_eval_accumulates_like_numpy():
    from wu.evaluate import EstimatorEval
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn((4, 5), generator=g), torch.randn((4, 5), generator=g)) for _ in range(3)]
    ev = EstimatorEval(lambda batch: batch)               # the "estimator" returns its input: pred = batch
    for pred, target in batches:
        ev.update(pred, target)
    diff = np.concatenate([(p - t).numpy() for p, t in batches]).astype(np.float64)
    res = ev.result()
    assert res["count"] == 12 and res["mean"].dtype == torch.float64
    np.testing.assert_allclose(res["mean"].numpy(), diff.mean(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res["std"].numpy(), diff.std(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res["mse"].numpy(), (diff ** 2).mean(0), rtol=1e-12, atol=1e-15)


def test_sweep_chunks_and_one_seed_draw_per_chunk():
    import cunet
    from wu.unet_graph import SWEEP_MAX_IMAGES, sweep_chunks, sweep_plan
    assert sweep_chunks(5, 16, 64) == [(0, 4), (4, 5)]                    # 64 // 16 = 4 rows per chunk
    assert sweep_chunks(3, 2, 4) == [(0, 2), (2, 3)]
    assert sweep_chunks(3, 8, 4) == [(0, 1), (1, 2), (2, 3)]              # never less than one row
    assert sweep_chunks(64, 2, 128) == [(0, 64)]
    assert sweep_chunks(5, 16) == sweep_chunks(5, 16, SWEEP_MAX_IMAGES)
    with pytest.raises(ValueError):
        sweep_chunks(0, 2, 4)

    class Counting(cunet.Conditional_UNet):
        drawn = None

        def _next_seed(self, k):
            self.drawn.append(k)
            return super()._next_seed(k)

    net = Counting(5)
    net.drawn = []
    plan = sweep_plan(net, 5, 2, 4)
    assert [(r0, r1) for r0, r1, _ in plan] == [(0, 2), (2, 4), (4, 5)]
    assert net.drawn == [3, 2, 1] * 3                                     # one triple per chunk, levels 3, 2, 1, chunk after chunk
    seeds = [s for _, _, s in plan]
    assert len({s for t in seeds for s in t}) == 9                        # fresh seeds: every draw differs
    net.dropout_seed = 7
    assert [s for _, _, s in sweep_plan(net, 5, 2, 4)] == [(7 * 4 + 3, 7 * 4 + 2, 7 * 4 + 1)] * 3     # a fixed seed: what forward() draws


def test_sweep_entry_points_reject_bad_arguments_without_a_gpu():
    from wu import _lib
    lib = _lib.load()
    A = 4096                         # any 16-byte aligned, non-null address: validation happens before anything is dereferenced

    def upcat(x=A, ldx=64, bx=2, skip=A, ldskip=64, bs=2, cs=64, y=A, ldy=128, n=6, c=64):
        return lib.wu_adain_upcat_sweep_fwd(x, ldx, bx, A, A, A, skip, ldskip, bs, cs, y, ldy, n, 3, 5, c, 0.0, 1, None, _lib.BF16, None)

    assert upcat(n=5) < 0 and b"Bx=2 must divide N=5" in lib.wu_last_error()
    assert upcat(bs=4) < 0 and b"Bs=4 must divide N=6" in lib.wu_last_error()
    assert upcat(x=A + 8) < 0 and b"alignment" in lib.wu_last_error()
    assert upcat(skip=A + 2) < 0 and b"alignment" in lib.wu_last_error()
    assert upcat(c=128, ldx=64) < 0 and b"<= ldx=64" in lib.wu_last_error()
    assert upcat(c=128, ldx=128, ldy=128) < 0 and b"fit ldy=128" in lib.wu_last_error()
    assert upcat(cs=64, ldskip=32) < 0 and b"<= ldskip=32" in lib.wu_last_error()

    def stats(x=A, ldx=512, n=2, c=512, split_batch=128):
        return lib.wu_adain_stats_as_batch(x, ldx, A, A, n, 17, 17, c, 1e-5, split_batch, _lib.BF16, None)

    assert stats(split_batch=127) < 0 and b"multiple of N=2" in lib.wu_last_error()
    assert stats(split_batch=1) < 0 and b"multiple of N=2" in lib.wu_last_error()
    assert stats(x=A + 4) < 0 and b"adain_stats" in lib.wu_last_error()
    assert stats(c=96, ldx=96) < 0 and b"C=96" in lib.wu_last_error()
