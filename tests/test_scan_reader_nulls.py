"""Nullable columns through the native in-order scan reader
(native/hipdf/scan_reader.hip): the validity mask comes from the definition
levels, decoded on the reader's worker threads, and one kernel per slice of
a page places the dense values. Every batch equals what pyarrow reads from
its files, and a query over such a scan equals the per-file path and the CPU
backend."""
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

pytestmark = pytest.mark.gpu

PAGE_ROWS = 20_000
PIECE = 64 << 10  # 16 384 four-byte values: a page spans two slices
DEC = pa.decimal128(7, 2)
COLS = ["i32", "i64", "dec", "f32", "f64", "fk"]
NULLABLE = COLS[:5]
ORDER = "abcde"
ROWS = {"a": 70_001, "b": 1, "c": 13, "d": 20_000, "e": 0}


def _opts(version):
    return dict(compression=None, use_dictionary=False,
                store_decimal_as_integer=True, max_rows_per_page=PAGE_ROWS,
                data_page_size=8 << 20, data_page_version=version)


def _fact(name: str, seed: int) -> pa.Table:
    """File a: 2% nulls in four columns, the first and the last row of a page
    among them, and f32 all null. b and c: small files with nulls. d: no null
    in any nullable column. e: no rows."""
    rows = ROWS[name]
    rng = np.random.default_rng(seed)
    unscaled = rng.integers(-9_999_999, 9_999_999, rows, endpoint=True)
    vals = {
        "i32": rng.integers(-2**31, 2**31 - 1, rows, dtype=np.int32,
                            endpoint=True),
        "i64": rng.integers(-2**63, 2**63 - 1, rows, dtype=np.int64,
                            endpoint=True),
        "dec": unscaled,
        "f32": rng.standard_normal(rows).astype(np.float32),
        "f64": rng.standard_normal(rows),
    }
    cols = {}
    for k, c in enumerate(NULLABLE):
        null = np.zeros(rows, dtype=bool)
        if name != "d":
            null = rng.random(rows) < 0.02
            for r in (0, PAGE_ROWS - 1, PAGE_ROWS, rows - 1):
                if 0 <= r < rows and (k + r) % 2 == 0:
                    null[r] = True
            if name == "a" and c == "f32":
                null[:] = True
            if name == "b":
                null[:] = k % 2 == 0
        if c == "dec":
            cols[c] = pa.array(
                [None if m else decimal.Decimal(int(v)).scaleb(-2)
                 for v, m in zip(vals[c], null)], type=DEC)
        else:
            cols[c] = pa.array(vals[c], mask=null)
    # 0..59: keys 50..59 miss the 50-row dimension
    cols["fk"] = pa.array(rng.integers(0, 60, rows, dtype=np.int32))
    return pa.table(cols)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Files a..e in both page versions, the dimension, and the pyarrow read
    of every fact file. Tests read these, never write."""
    d = tmp_path_factory.mktemp("scan_reader_nulls")
    out = {"files": {}, "arrow": {}}
    for version in ("1.0", "2.0"):
        for seed, name in enumerate(ORDER):
            p = str(d / f"{name}{version[0]}.parquet")
            pq.write_table(_fact(name, seed + 1), p, **_opts(version))
            out["files"][name + version[0]] = p
            out["arrow"][name + version[0]] = pq.read_table(p)
    a = out["arrow"]["a1"]
    assert a["f32"].null_count == ROWS["a"] and a["dec"].null_count > 1000
    assert all(out["arrow"]["d1"][c].null_count == 0 for c in COLS)
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
        assert np.array_equal(got_valid, valid), name  # validity is exact
        got = c.to_numpy()
        assert got.dtype == vals.dtype, (name, got.dtype, vals.dtype)
        # bit-exact at valid rows, floats included
        assert np.array_equal(got[valid].view(np.uint8),
                              vals[valid].view(np.uint8)), name
        # the data at null rows is zero
        assert not got[~valid].view(np.uint8).any(), name


def _table(paths, threads, per_batch):
    from spark_rapids_amd.io.parquet import ParquetTable

    return ParquetTable(list(paths), reader="GPU_DECODE",
                        prefetch_threads=threads, columns=COLS,
                        stream_scan=True, stream_files=per_batch,
                        stream_piece_bytes=PIECE, stream_nulls=True)


def _stats():
    from spark_rapids_amd.io.parquet import SCAN_STATS

    return dict(SCAN_STATS)


def _paths(data, v, names=ORDER):
    return [data["files"][n + v] for n in names]


@pytest.mark.parametrize("v", ["1", "2"])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("per_batch", [1, 2, 5])
def test_batches_equal_pyarrow(data, v, threads, per_batch):
    """With 2 and 5 files per batch the 70 001-row file is followed by
    another file in the same batch, whose mask starts inside a byte."""
    import torch

    before = _stats()
    batches = list(_table(_paths(data, v), threads, per_batch).partitions())
    torch.cuda.synchronize()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"] + 1
    assert after["stream_scans_not_eligible"] == \
        before["stream_scans_not_eligible"]
    assert after["fallback_files"] == before["fallback_files"]
    groups = [ORDER[i:i + per_batch] for i in range(0, len(ORDER), per_batch)]
    assert len(batches) == len(groups)
    for batch, group in zip(batches, groups):
        _assert_batch_equals(batch, [data["arrow"][n + v] for n in group])
    if per_batch == 5:
        # the footers' null counts add up to the column's
        want = pa.concat_tables([data["arrow"][n + v] for n in ORDER])
        for name, c in zip(COLS, batches[0].columns):
            assert c.null_count == want[name].null_count, name
            assert (c.validity is None) == (want[name].null_count == 0), name


def test_file_order_moves_the_bit_offsets(data):
    """The small files first: every later file starts at another bit."""
    import torch

    names = "cbad"
    batches = list(_table(_paths(data, "1", names), 3, 4).partitions())
    torch.cuda.synchronize()
    assert len(batches) == 1
    _assert_batch_equals(batches[0], [data["arrow"][n + "1"] for n in names])


def test_nulls_off_takes_the_per_file_path(data):
    import torch

    from spark_rapids_amd.io.parquet import ParquetTable

    before = _stats()
    t = ParquetTable(_paths(data, "1", "abc"), reader="GPU_DECODE",
                     prefetch_threads=3, columns=COLS, stream_scan=True,
                     stream_files=1, stream_piece_bytes=PIECE)
    batches = list(t.partitions())
    torch.cuda.synchronize()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"]
    assert after["stream_scans_not_eligible"] == \
        before["stream_scans_not_eligible"] + 1
    for batch, n in zip(batches, "abc"):
        _assert_batch_equals(batch, [data["arrow"][n + "1"]])


def test_consumer_that_stops_early_then_a_second_scan(data):
    import torch

    paths = _paths(data, "2", "abcd")
    it = _table(paths, 3, 1).partitions()
    first = next(it)
    it.close()  # the rest is cancelled
    torch.cuda.synchronize()
    _assert_batch_equals(first, [data["arrow"]["a2"]])
    del first
    batches = list(_table(paths, 3, 1).partitions())
    torch.cuda.synchronize()
    assert len(batches) == 4
    for batch, n in zip(batches, "abcd"):
        _assert_batch_equals(batch, [data["arrow"][n + "2"]])


def test_twenty_scans_do_not_grow_device_memory(data):
    import torch

    from spark_rapids_amd.tools.memwatch import assert_no_leak

    paths = _paths(data, "1")
    rows = sum(ROWS.values())
    list(_table(paths, 3, 2).partitions())  # opens the reader
    torch.cuda.synchronize()
    with assert_no_leak():
        for _ in range(20):
            got = sum(b.num_rows for b in _table(paths, 3, 2).partitions())
            assert got == rows
        torch.cuda.synchronize()


# ---- query level -----------------------------------------------------------

def _query(session, data):
    from spark_rapids_amd import col, sum_
    from spark_rapids_amd.expr.aggregates import avg, count, count_star

    fact = session.read_parquet(_paths(data, "1"), columns=COLS)
    dim = session.read_parquet(data["dim"], replicated=True)
    return (fact.join(dim, on="fk", right_on=["d_sk"])
            .group_by("d_name", "d_class")
            .agg(sum_(col("dec")).alias("s"), avg(col("dec")).alias("ad"),
                 count(col("dec")).alias("cd"), avg(col("f64")).alias("a"),
                 count(col("f32")).alias("cf"), count_star().alias("n"))
            .sort("d_name", "d_class")
            .limit(40))


def _session(enabled=True, nulls=True, per_batch=2):
    from spark_rapids_amd import Session

    return Session({
        "spark.rapids.sql.enabled": enabled,
        "spark.rapids.sql.format.parquet.streamScan.nulls.enabled": nulls,
        "spark.rapids.sql.format.parquet.streamScan.filesPerBatch": per_batch,
    })


def _assert_rows_equal(got, want):
    assert len(got) == len(want) and len(want) > 10
    for g, w in zip(got, want):
        assert len(g) == len(w) == 8
        for i, (x, y) in enumerate(zip(g, w)):
            if isinstance(y, float):
                # float averages, as the existing query test compares them
                assert abs(x - y) <= 1e-12 * abs(y), (i, g, w)
            else:
                # keys, decimal sums and counts are exact
                assert x == y, (i, g, w)


def test_query_conf_on_conf_off_and_cpu_agree(data):
    cpu = _query(_session(enabled=False), data).collect()
    # the all-null f32 of file a is counted nowhere, every row is counted
    assert sum(r[7] for r in cpu) > sum(r[6] for r in cpu) > 0

    before = _stats()
    on = _query(_session(), data).collect()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"] + 1
    assert after["stream_scans_not_eligible"] == \
        before["stream_scans_not_eligible"]
    _assert_rows_equal(on, cpu)

    before = _stats()
    off = _query(_session(nulls=False), data).collect()
    after = _stats()
    assert after["stream_scans"] == before["stream_scans"]
    assert after["stream_scans_not_eligible"] == \
        before["stream_scans_not_eligible"] + 1
    _assert_rows_equal(off, cpu)
