"""_exclusive_scan_i64 through the one-call native scan (every level
enqueued by hipdf_exclusive_scan_i64, total in the last scratch slot):
output and total must equal np.cumsum exactly at every level boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# one scan block covers 2048 elements; 2048^2 + 5 forces three levels
SIZES = [0, 1, 2047, 2048, 2049, 2048 ** 2 - 1, 2048 ** 2 + 5]


@pytest.mark.parametrize("n", SIZES)
def test_exclusive_scan_matches_cumsum(n):
    from spark_rapids_amd.ops import gpu_backend

    rng = np.random.default_rng(n + 3)
    vals = rng.integers(0, 1000, n).astype(np.int64)
    out, total = gpu_backend._exclusive_scan_i64(torch.from_numpy(vals).cuda())
    incl = np.cumsum(vals)
    assert isinstance(total, int)
    assert total == (int(incl[-1]) if n else 0)
    assert out.numel() == n
    if n:
        assert np.array_equal(out.cpu().numpy(), incl - vals)


def test_scratch_size_and_levels():
    import hipdf as ext

    per = 2048
    assert ext.scan_scratch_elems(1) == 1
    assert ext.scan_scratch_elems(per) == 1
    # two levels: sums + their scan (2 each) and the total slot
    assert ext.scan_scratch_elems(per + 1) == 2 * 2 + 1
    assert ext.scan_scratch_elems(per * per) == 2 * per + 1
    # three levels
    assert ext.scan_scratch_elems(per * per + 5) == 2 * (per + 1) + 2 * 2 + 1
