"""GPU: the one device-to-host fetch the image encoders share (wu/_codec.py fetch_packed), on a buffer whose every byte is known."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_fetch_packed_returns_the_used_bytes_of_the_named_slots_and_reuses_its_buffer():
    from wu import _codec
    out = torch.arange(3 * 64, dtype=torch.uint8, device=DEV)               # 3 slots, stride 64
    pool = _codec.StagingPool(8)
    want = [bytes(range(0, 5)), bytes(range(128, 192))]
    with torch.cuda.device(DEV):
        for _ in range(2):
            assert _codec.fetch_packed(pool, out, 64, [5, 17, 64], [0, 2]) == want
            assert len(pool) == 1                                           # the second call found the first buffer's event complete
        assert _codec.fetch_packed(pool, out, 64, [5, 17, 64]) == [bytes(range(0, 5)), bytes(range(64, 81)), bytes(range(128, 192))]
        assert _codec.fetch_packed(pool, out, 64, [5, 17, 64], []) == [] and len(pool) == 1
    (st,) = pool._buffers
    assert not st.held and st.event.query() and st.tensor.is_pinned()
