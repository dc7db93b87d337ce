"""The native in-order scan reader (native/hipdf/scan_reader.hip) behind a
multi-file GPU_DECODE scan: every batch is a group of files, equal to what
pyarrow reads from them, and a query over such a scan equals the per-file
path and the CPU backend."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

pytestmark = pytest.mark.gpu

PAGE_ROWS = 20_000
PIECE = 64 << 10
DEC = pa.decimal128(7, 2)
COLS = ["i32", "i64", "dec", "f32", "f64", "fk"]
_OPTS = dict(compression=None, use_dictionary=False,
             store_decimal_as_integer=True, max_rows_per_page=PAGE_ROWS,
             data_page_size=8 << 20)


def _fact(rows: int, seed: int) -> pa.Table:
    rng = np.random.default_rng(seed)
    unscaled = rng.integers(-9_999_999, 9_999_999, rows, endpoint=True)
    if rows >= 2:
        unscaled[0], unscaled[-1] = -9_999_999, 9_999_999
    dec = pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in unscaled],
                   type=DEC)
    return pa.table({
        "i32": pa.array(rng.integers(-2**31, 2**31 - 1, rows, dtype=np.int32,
                                     endpoint=True)),
        "i64": pa.array(rng.integers(-2**63, 2**63 - 1, rows, dtype=np.int64,
                                     endpoint=True)),
        "dec": dec,
        "f32": pa.array(rng.standard_normal(rows).astype(np.float32)),
        "f64": pa.array(rng.standard_normal(rows)),
        # 0..59: keys 50..59 miss the 50-row dimension
        "fk": pa.array(rng.integers(0, 60, rows, dtype=np.int32)),
    })


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Files a..e (70 001, 1, 20 000, 0 and 20 000 rows), a file with nulls,
    a file with a dictionary column, the dimension, and the pyarrow read of
    every fact file. Tests read these, never write."""
    d = tmp_path_factory.mktemp("scan_reader")
    out = {"files": {}, "arrow": {}}
    for name, rows, seed in (("a", 70_001, 1), ("b", 1, 2), ("c", 20_000, 3),
                             ("d", 0, 4), ("e", 20_000, 5)):
        p = str(d / f"{name}.parquet")
        pq.write_table(_fact(rows, seed), p, **_OPTS)
        out["files"][name] = p
    t = _fact(20_000, 6)
    mask = np.zeros(20_000, dtype=bool)
    mask[::50] = True
    t = t.set_column(0, "i32", pa.array(t["i32"].to_numpy(), mask=mask))
    p = str(d / "nulls.parquet")
    pq.write_table(t, p, **_OPTS)
    out["files"]["nulls"] = p
    p = str(d / "dict.parquet")
    pq.write_table(_fact(20_000, 7), p,
                   **{**_OPTS, "use_dictionary": ["fk"]})
    out["files"]["dict"] = p
    for name, p in out["files"].items():
        out["arrow"][name] = pq.read_table(p)
    dim = pa.table({
        "d_sk": pa.array(np.arange(50, dtype=np.int32)),
        "d_name": pa.array([f"name-{i % 9}" for i in range(50)]),
        "d_class": pa.array((np.arange(50) % 4 + 7).astype(np.int32)),
    })
    out["dim"] = str(d / "dim.parquet")
    pq.write_table(dim, out["dim"], compression=None, use_dictionary=True)
    return out


def _arrow_np(tbl: pa.Table, name: str):
    """(values, valid) of a pyarrow column; decimals as unscaled int64."""
    arr = tbl[name].combine_chunks()
    valid = ~np.asarray(arr.is_null())
    if pa.types.is_decimal(arr.type):
        arr = pa.concat_arrays([arr])
        raw = np.frombuffer(arr.buffers()[1], dtype=np.int64,
                            count=2 * len(arr))
        return raw[0::2].copy(), valid
    return arr.fill_null(0).to_numpy(zero_copy_only=False), valid


def _assert_batch_equals(batch, tables):
    want = pa.concat_tables(tables)
    assert batch.num_rows == want.num_rows
    for name, c in zip(COLS, batch.columns):
        vals, valid = _arrow_np(want, name)
        c = c.cpu()
        got_valid = np.asarray(c.valid_array())
        assert np.array_equal(got_valid, valid), name
        got = c.to_numpy()
        assert got.dtype == vals.dtype, (name, got.dtype, vals.dtype)
        # bit-exact, floats included
        assert np.array_equal(got[valid].view(np.uint8),
                              vals[valid].view(np.uint8)), name


def _table(paths, threads, per_batch, stream=True):
    from spark_rapids_amd.io.parquet import ParquetTable

    return ParquetTable(list(paths), reader="GPU_DECODE",
                        prefetch_threads=threads, columns=COLS,
                        stream_scan=stream, stream_files=per_batch,
                        stream_piece_bytes=PIECE)


def _stats():
    from spark_rapids_amd.io.parquet import SCAN_STATS

    return dict(SCAN_STATS)


@pytest.mark.parametrize("names", ["abc", "abdce"])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("per_batch", [1, 2])
def test_batches_are_the_file_groups(data, names, threads, per_batch):
    """abc: the three base files; abdce: more files than threads, with the
    0-row file among them."""
    import torch

    before = _stats()
    t = _table([data["files"][n] for n in names], threads, per_batch)
    batches = list(t.partitions())
    torch.cuda.synchronize()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"] + 1
    assert after["fallback_files"] == before["fallback_files"]
    groups = [names[i:i + per_batch] for i in range(0, len(names), per_batch)]
    assert len(batches) == len(groups)
    for batch, group in zip(batches, groups):
        _assert_batch_equals(batch, [data["arrow"][n] for n in group])


def test_consumer_that_stops_early_then_a_second_scan(data):
    import torch

    paths = [data["files"][n] for n in "abce"]
    it = _table(paths, 3, 1).partitions()
    first = next(it)
    it.close()  # the rest is cancelled
    torch.cuda.synchronize()
    _assert_batch_equals(first, [data["arrow"]["a"]])
    del first
    batches = list(_table(paths, 3, 1).partitions())
    assert len(batches) == 4
    for batch, n in zip(batches, "abce"):
        _assert_batch_equals(batch, [data["arrow"][n]])


def test_twenty_scans_do_not_grow_device_memory(data):
    import torch

    from spark_rapids_amd.tools.memwatch import assert_no_leak

    paths = [data["files"][n] for n in "abdce"]
    rows = sum(data["arrow"][n].num_rows for n in "abdce")
    list(_table(paths, 3, 2).partitions())  # opens the reader
    torch.cuda.synchronize()
    with assert_no_leak():
        for _ in range(20):
            got = sum(b.num_rows for b in _table(paths, 3, 2).partitions())
            assert got == rows
        torch.cuda.synchronize()


@pytest.mark.parametrize("odd", ["nulls", "dict"])
def test_ineligible_file_takes_the_per_file_path(data, odd):
    import torch

    names = ["a", odd, "c"]
    before = _stats()
    batches = list(_table([data["files"][n] for n in names], 3, 1)
                   .partitions())
    torch.cuda.synchronize()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"]
    assert after["stream_scans_not_eligible"] == \
        before["stream_scans_not_eligible"] + 1
    assert after["fallback_files"] == before["fallback_files"]
    assert len(batches) == 3  # one per file, as before
    for batch, n in zip(batches, names):
        _assert_batch_equals(batch, [data["arrow"][n]])


# ---- query level -----------------------------------------------------------

def _query(session, data, names):
    from spark_rapids_amd import col, sum_
    from spark_rapids_amd.expr.aggregates import avg, count_star

    fact = session.read_parquet([data["files"][n] for n in names],
                                columns=COLS)
    dim = session.read_parquet(data["dim"], replicated=True)
    return (fact.join(dim, on="fk", right_on=["d_sk"])
            .filter(col("f64") > -0.5)
            .group_by("d_name", "d_class")
            .agg(sum_(col("dec")).alias("s"), avg(col("f64")).alias("a"),
                 count_star().alias("n"))
            .sort("d_name", "d_class")
            .limit(30))


def _session(enabled=True, stream=True, per_batch=1):
    from spark_rapids_amd import Session

    return Session({
        "spark.rapids.sql.enabled": enabled,
        "spark.rapids.sql.format.parquet.streamScan.enabled": stream,
        "spark.rapids.sql.format.parquet.streamScan.filesPerBatch": per_batch,
    })


@pytest.fixture(scope="module")
def cpu_rows(data):
    return _query(_session(enabled=False), data, "abdce").collect()


def _assert_rows_equal(got, want):
    assert len(got) == len(want) and len(want) > 10
    for g, w in zip(got, want):
        # keys, the decimal sum and the count are exact
        assert g[:3] == w[:3] and g[4] == w[4], (g, w)
        assert abs(g[3] - w[3]) <= 1e-12 * abs(w[3]), (g, w)


def test_query_conf_on_conf_off_and_cpu_agree(data, cpu_rows, monkeypatch):
    from spark_rapids_amd.ops import gpu_backend as gb

    tables = []
    ranges = []
    real_table, real_minmax = gb._build_dict_group_table, gb._column_minmax

    def count_table(dicts, need_null_slot):
        tables.append(dicts[0].size)
        return real_table(dicts, need_null_slot)

    def count_minmax(k):
        ranges.append(k.size)
        return real_minmax(k)

    monkeypatch.setattr(gb, "_build_dict_group_table", count_table)
    monkeypatch.setattr(gb, "_column_minmax", count_minmax)

    before = _stats()
    on = _query(_session(per_batch=1), data, "abdce").collect()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"] + 1
    _assert_rows_equal(on, cpu_rows)
    # four non-empty fact batches went through the join and the partial
    # aggregate: the dimension's strings were grouped once, and the integer
    # key's range was found once, on the 50-row build column
    assert tables == [50], tables
    assert ranges.count(50) == 1, ranges
    on_calls = len(ranges)

    del tables[:], ranges[:]
    one = _query(_session(per_batch=5), data, "abdce").collect()
    _assert_rows_equal(one, cpu_rows)
    # the same number of range reductions with one batch as with four
    assert tables == [50] and len(ranges) == on_calls, (tables, ranges)

    before = _stats()
    off = _query(_session(stream=False), data, "abdce").collect()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"]
    assert after["stream_scans_not_eligible"] == \
        before["stream_scans_not_eligible"]
    _assert_rows_equal(off, cpu_rows)
