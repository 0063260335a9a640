"""CPU: the host plumbing the image codecs share (wu/_codec.py) -- the staging-buffer rule against stub events that record what was
asked of them, the encoders' batch geometry against ``Tensor.stride()`` written out by hand, and the plan cache's eviction order."""
import queue
import threading

import pytest
import torch

from wu import _codec, _lib

MIB = 1 << 20


class Event:
    """Stands in for torch.cuda.Event: ``done`` is what query() answers; every call is appended to ``log``."""
    def __init__(self, name, done, log):
        self.name, self.done, self.log = name, done, log

    def query(self):
        self.log.append(("query", self.name))
        return self.done

    def synchronize(self):
        self.log.append(("synchronize", self.name))
        self.done = True


def _busy_pool(n, log):
    """A pool of ``n`` buffers, all released, each behind an event that has not completed; buffer i carries event i."""
    pool = _codec.StagingPool(n)
    bufs = [pool.acquire(100) for _ in range(n)]
    for i, s in enumerate(bufs):
        s.event = Event(i, False, log)
        pool.release(s)
    return pool, bufs


def test_a_released_buffer_without_an_event_is_reused():
    pool = _codec.StagingPool(8)
    a = pool.acquire(100)
    assert a.held and a.event is None and not a.tensor.is_pinned() and a.tensor.numel() == MIB and len(pool) == 1
    pool.release(a)
    assert not a.held
    assert pool.acquire(MIB) is a and a.held and len(pool) == 1            # the same object, up to its full size


def test_a_held_buffer_is_never_handed_out_twice():
    pool = _codec.StagingPool(8)
    a = pool.acquire(100)
    b = pool.acquire(100)
    assert b is not a and len(pool) == 2
    pool.release(b)
    assert pool.acquire(100) is b and len(pool) == 2                        # and never a, which is still held


def test_a_buffer_whose_event_has_not_completed_is_not_reused():
    log = []
    pool = _codec.StagingPool(8)
    a = pool.acquire(100)
    a.event = Event("a", False, log)
    pool.release(a)
    b = pool.acquire(100)
    assert b is not a and len(pool) == 2 and log == [("query", "a")]        # asked on the host, never waited for
    a.event.done = True
    assert pool.acquire(100) is a and len(pool) == 2


def test_a_full_pool_waits_for_the_oldest_event_only_then_allocates(monkeypatch):
    log = []
    pool, bufs = _busy_pool(3, log)

    class Logged(_codec.Staging):
        def __init__(self, nbytes, pinned):
            log.append(("allocate", nbytes))
            super().__init__(nbytes, pinned)

    monkeypatch.setattr(_codec, "Staging", Logged)
    new = pool.acquire(100)
    assert log == [("query", 0), ("query", 1), ("query", 2), ("synchronize", 0), ("allocate", MIB)]
    assert len(pool) == 3 and new not in bufs and new.held
    assert pool._buffers == [bufs[1], bufs[2], new]                         # the oldest left the pool


def test_a_full_pool_grows_when_every_buffer_is_held():
    pool = _codec.StagingPool(2)
    held = [pool.acquire(100) for _ in range(3)]
    assert len(pool) == 3 and len({id(s) for s in held}) == 3 and all(s.held for s in held)


def test_a_request_larger_than_any_buffer_gets_a_new_one_with_headroom():
    pool = _codec.StagingPool(8)
    small = pool.acquire(100)
    pool.release(small)
    n = 3 * MIB + 1
    big = pool.acquire(n)
    assert big is not small and big.tensor.numel() == max(int(1.25 * n), MIB) == int(1.25 * n) and len(pool) == 2
    assert small.tensor.numel() == max(int(1.25 * 100), MIB) == MIB
    pool.clear()
    assert len(pool) == 0 and not pool


def test_release_from_a_second_thread_while_the_first_acquires():
    pool = _codec.StagingPool(2)
    handed = queue.Queue(maxsize=4)

    def releaser():
        while True:
            s = handed.get()
            if s is None:
                return
            s.owner = None                    # before the release: after it the buffer may be handed out again at once
            pool.release(s)

    t = threading.Thread(target=releaser)
    t.start()
    try:
        for i in range(2000):
            s = pool.acquire(100)
            assert s.held and getattr(s, "owner", None) is None, f"round {i}: a held buffer was handed out"
            s.owner = i
            handed.put(s)
    finally:
        handed.put(None)
        t.join()
    assert len(pool) <= 6 and not any(s.held for s in pool._buffers)        # at most 4 queued, 1 with each thread


def test_host_batch_releases_its_buffer_once_and_upload_refuses_a_released_one():
    pool = _codec.StagingPool(2)
    hb = _codec.HostBatch(pool)
    hb.staging = pool.acquire(100)
    st = hb.staging
    hb.release()
    hb.release()
    assert hb.staging is None and not st.held
    with pytest.raises(RuntimeError, match="Who: this HostBatch was released"):
        _codec.upload(hb, torch.device("cpu"), "Who")
    hb.staging = pool.acquire(100)
    del hb                                    # garbage collection releases too
    assert not st.held


GEOMETRY = {
    # name: (tensor, dtype code, N, H, W, element strides (n, c, y, x)) with the strides written out by hand
    "u8_nhwc": (lambda: torch.zeros(2, 4, 5, 3, dtype=torch.uint8), _codec.U8, 2, 4, 5, (60, 1, 15, 3)),
    "u8_slice": (lambda: torch.zeros(2, 6, 7, 3, dtype=torch.uint8)[:, 1:-1, ::2], _codec.U8, 2, 4, 4, (126, 1, 21, 6)),
    "f32_nchw": (lambda: torch.zeros(2, 3, 4, 5), _lib.F32, 2, 4, 5, (60, 20, 5, 1)),
    "f32_channels_last": (lambda: torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last), _lib.F32, 2, 4, 5, (60, 1, 15, 3)),
    "bf16_nchw": (lambda: torch.zeros(1, 3, 2, 9, dtype=torch.bfloat16), _lib.BF16, 1, 2, 9, (54, 18, 9, 1)),
}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_batch_geometry_reports_the_strides_of_the_tensor(name):
    make, dt, n, h, w, strides = GEOMETRY[name]
    x = make()
    assert _codec.batch_geometry(x, "Who") == (dt, n, h, w, strides)
    s = x.stride()
    assert strides == ((s[0], s[3], s[1], s[2]) if x.dtype == torch.uint8 else tuple(s))
    assert _codec.U8 == 2 and len({_codec.U8, _lib.F32, _lib.BF16}) == 3
    assert _codec.check_sizes(n, h, w, None, strides, "Who") == [(h, w)] * n


def test_batch_geometry_and_check_sizes_refuse_bad_batches():
    with pytest.raises(ValueError, match="Who: images must be a 4-d tensor"):
        _codec.batch_geometry(torch.zeros(8, 8, 3, dtype=torch.uint8), "Who")
    with pytest.raises(ValueError, match="Who: images must be a 4-d tensor"):
        _codec.batch_geometry([[0]], "Who")
    with pytest.raises(ValueError, match=r"Who: a uint8 batch is \(N,H,W,3\), got \(1, 8, 8, 4\)"):
        _codec.batch_geometry(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), "Who")
    with pytest.raises(ValueError, match=r"Who: a float batch is \(N,3,H,W\), got \(1, 8, 8, 3\)"):
        _codec.batch_geometry(torch.zeros(1, 8, 8, 3), "Who")
    with pytest.raises(ValueError, match="Who: dtype torch.float16 is not uint8 / float32 / bfloat16"):
        _codec.batch_geometry(torch.zeros(1, 3, 8, 8, dtype=torch.float16), "Who")
    ok = (60, 1, 15, 3)
    with pytest.raises(ValueError, match="Who: negative strides"):
        _codec.check_sizes(2, 4, 5, None, (60, 1, -15, 3), "Who")
    with pytest.raises(ValueError, match="Who: empty batch"):
        _codec.check_sizes(0, 4, 5, None, ok, "Who")
    with pytest.raises(ValueError, match="Who: sizes must be 2 pairs"):
        _codec.check_sizes(2, 4, 5, [(4, 5)], ok, "Who")
    with pytest.raises(ValueError, match="inside the batch's 4 x 5"):
        _codec.check_sizes(2, 4, 5, [(4, 5), (5, 5)], ok, "Who")
    with pytest.raises(ValueError, match="inside the batch's 4 x 5"):
        _codec.check_sizes(2, 4, 5, [(4, 5), (4, 0)], ok, "Who")
    assert _codec.check_sizes(2, 4, 5, [(4.0, 5), (1, 1)], ok, "Who") == [(4, 5), (1, 1)]


def test_plan_cache_evicts_in_insertion_order_and_a_hit_does_not_reorder():
    cache = _codec.PlanCache("Who", "the descriptors")
    built = []

    def get(key):
        return cache.get(key, lambda: built.append(key) or ("plan", key))

    for k in range(64):
        assert get(k) == ("plan", k)
    assert len(cache) == 64 and built == list(range(64))
    assert get(0) == ("plan", 0) and built == list(range(64))               # a hit: nothing built, nothing moved
    assert get(64) == ("plan", 64) and len(cache) == 64                     # the 65th key
    assert 0 not in cache and 1 in cache and 64 in cache                    # the first one inserted left, hit or not
    assert get(0) == ("plan", 0) and built == list(range(65)) + [0] and 1 not in cache


def test_small_helpers(tmp_path):
    assert [_codec.align(v) for v in (0, 1, 256, 257)] == [0, 256, 256, 512] and _codec.align(17, 16) == 32
    assert _codec.worker_threads(0) == 1 and _codec.worker_threads(3) == 3 and _codec.worker_threads(99) == _codec.MAX_THREADS == 16
    assert 1 <= _codec.worker_threads(None) <= 16
    p = tmp_path / "x.bin"
    _codec.write((str(p), b"abc"))
    assert _codec.read(p) == b"abc" == _codec.read(bytearray(b"abc")) and _codec.name(p) == str(p) and _codec.name(b"", 3) == "<bytes #3>"
    with pytest.raises(RuntimeError, match="cannot decode image x.bin"):
        _codec.pillow_rgb(b"abc", "x.bin")
    stats, lock = {"native": 0, "fallback": 0, "fallback_reasons": {}}, threading.Lock()
    for reason in (None, "a", "a", "b"):
        _codec.count(stats, lock, reason)
    assert stats == {"native": 1, "fallback": 3, "fallback_reasons": {"a": 2, "b": 1}}
