"""Host counterparts of the join build/probe split: building once and
probing per batch gives what join_gather_maps gives, through the dispatcher
and through a multi-batch HashJoinExec."""
import numpy as np
import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, ColumnBatch, ops
from spark_rapids_amd.types import FLOAT64, INT32


def _batches():
    rng = np.random.default_rng(3)
    n, nbuild = 500, 60
    left = ColumnBatch([
        Column.from_numpy(rng.integers(0, 90, n).astype(np.int32), INT32,
                          rng.random(n) >= 0.1),
        Column.from_numpy(np.arange(n, dtype=np.float64), FLOAT64)], n)
    right = ColumnBatch([
        Column.from_numpy(rng.permutation(nbuild).astype(np.int32), INT32),
        Column.from_numpy(np.arange(nbuild, dtype=np.int32), INT32)], nbuild)
    return left, right


@pytest.mark.parametrize("how", ["inner", "left", "semi", "anti", "full"])
def test_build_probe_equals_gather_maps(how):
    left, right = _batches()
    want_matched = np.zeros(right.num_rows, dtype=bool)
    got_matched = np.zeros(right.num_rows, dtype=bool)
    lw, rw = ops.join_gather_maps(left, right, [0], [0], how, want_matched)
    table = ops.join_build_table(right, [0])
    lg, rg = ops.join_probe(table, left, [0], how, got_matched)
    assert lg.to_pylist() == lw.to_pylist()
    assert (rg is None) == (rw is None)
    if rw is not None:
        assert rg.to_pylist() == rw.to_pylist()
    assert np.array_equal(want_matched, got_matched)


def test_multi_batch_left_join_cpu():
    s = sr.Session({"spark.rapids.sql.enabled": False})
    k = np.arange(300, dtype=np.int32) % 70
    left = s.create_dataframe({"k": k, "a": np.arange(300, dtype=np.float64)},
                              num_partitions=3)
    right = s.create_dataframe({"k": np.arange(50, dtype=np.int32),
                                "b": np.arange(50, dtype=np.int32) * 2})
    out = sorted(left.join(right, on="k").collect())
    want = sorted((int(x), float(i), int(x) * 2)
                  for i, x in enumerate(k) if x < 50)
    assert out == want
