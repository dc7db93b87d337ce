"""Host-to-device upload path of the GPU parquet reader: ext.memcpy_h2d
(GIL released, callable from several threads at once) and the
_upload_parts / _upload_array helpers built on it. Every check reads the
device buffer back and compares exact bytes."""
import threading

import numpy as np
import pytest

KIB = 1 << 10
MIB = 1 << 20

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_bytes():
    """2 MiB + change of reproducible bytes; tests slice it, never write."""
    rng = np.random.default_rng(20260)
    a = rng.integers(0, 256, 2 * MIB + 64, dtype=np.uint8)
    a.setflags(write=False)
    return a


def _upload(parts, **kw):
    import torch

    from spark_rapids_amd.io.parquet_gpu import _upload_parts
    from spark_rapids_amd.ops.gpu_backend import ext

    return _upload_parts(parts, ext,
                         torch.cuda.current_stream().cuda_stream, **kw)


def _readback(dev):
    import torch

    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("nbytes", [0, 1, 64 * KIB - 1, 64 * KIB,
                                    64 * KIB + 1, MIB, 2 * MIB + 17])
def test_exact_bytes_sizes(host_bytes, nbytes):
    src = host_bytes[:nbytes]
    got = _readback(_upload([src]))
    assert got.dtype == np.uint8 and got.shape == (nbytes,)
    assert np.array_equal(got, src)


@pytest.mark.parametrize("shift", [1, 3, 7])
def test_exact_bytes_odd_source_address(host_bytes, shift):
    src = host_bytes[shift:shift + MIB + 5]
    assert src.ctypes.data % 2 == 1
    assert np.array_equal(_readback(_upload([src])), src)


def test_multi_part_matches_concatenation(host_bytes):
    # empty parts between full ones, many small parts, odd starts, and
    # bytes objects next to arrays as the page parser hands them over
    cuts = [(0, 0), (5, 64 * KIB), (0, 0), (64 * KIB + 5, 64 * KIB + 6),
            (70_001, 70_001 + 128 * KIB + 11), (0, 0)]
    cuts += [(300_000 + 7 * i, 300_000 + 7 * i + (i % 5)) for i in range(60)]
    cuts += [(MIB + 1, MIB + 1 + 320 * KIB), (9, 10)]
    parts = [host_bytes[a:b] for a, b in cuts]
    want = np.concatenate(parts)
    mixed = [p.tobytes() if i % 3 == 0 else p for i, p in enumerate(parts)]
    assert np.array_equal(_readback(_upload(mixed)), want)


def test_pad_and_dtype_view(host_bytes):
    import torch

    src = host_bytes[3:3 + 4 * 1000]
    got = _upload([src[:1600], src[1600:]], torch_dtype=torch.int32)
    assert got.dtype == torch.int32 and got.numel() == 1000
    assert np.array_equal(_readback(got), src.copy().view("<i4"))
    padded = _readback(_upload([src[:999]], pad=8))
    assert padded.shape == (999 + 8,)
    assert np.array_equal(padded[:999], src[:999])
    assert not padded[999:].any()


def test_upload_array_keeps_dtype():
    import torch

    from spark_rapids_amd.io.parquet_gpu import _upload_array
    from spark_rapids_amd.ops.gpu_backend import ext

    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    for dt in (np.int32, np.int64):
        a = rng.integers(-2**31, 2**31, 100_003).astype(dt)
        for src in (a, a[:-1], a[1:]):  # views as _byte_array_dense passes
            got = _upload_array(src, ext, s)
            assert got.dtype == torch.from_numpy(a[:0]).dtype
            assert np.array_equal(_readback(got), src)
    assert _upload_array(np.empty(0, np.int64), ext, s).numel() == 0


def test_source_may_be_reused_on_return(host_bytes):
    src = host_bytes[11:11 + MIB].copy()
    want = src.copy()
    dev = _upload([src])
    src[:] = 0xFF  # the call has returned: the source is ours again
    assert np.array_equal(_readback(dev), want)


def test_upload_counts_bytes_and_time(host_bytes):
    from spark_rapids_amd.io.parquet import PHASE_STATS

    b0, t0 = PHASE_STATS["upload_bytes"], PHASE_STATS["upload_s"]
    _upload([host_bytes[:MIB], host_bytes[5:105]], pad=8)
    assert PHASE_STATS["upload_bytes"] - b0 == MIB + 100  # pad not counted
    assert PHASE_STATS["upload_s"] > t0


def test_concurrent_uploads_distinct_streams():
    """Four threads, each on its own stream, inside memcpy_h2d at once
    (the binding holds no GIL): every buffer must still be exact."""
    import hipdf
    import torch

    n_threads, rounds, nbytes = 4, 20, 320 * KIB + 123
    devs = [[torch.empty(nbytes, dtype=torch.uint8, device="cuda")
             for _ in range(rounds)] for _ in range(n_threads)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    start = threading.Barrier(n_threads)
    errors = []

    def pattern(t, r):
        return ((np.arange(nbytes, dtype=np.uint32) * (2 * t + 3)
                 + 31 * r + t) & 0xFF).astype(np.uint8)

    def work(t):
        try:
            src = np.empty(nbytes, dtype=np.uint8)
            start.wait()
            for r in range(rounds):
                src[:] = pattern(t, r)
                rc = hipdf.memcpy_h2d(devs[t][r].data_ptr(), src.ctypes.data,
                                      nbytes, streams[t].cuda_stream)
                assert rc == 0, rc
            streams[t].synchronize()
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append((t, e))
            start.abort()

    threads = [threading.Thread(target=work, args=(t,))
               for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for t in range(n_threads):
        for r in range(rounds):
            assert np.array_equal(devs[t][r].cpu().numpy(), pattern(t, r)), \
                (t, r)


def test_reader_path_matches_pyarrow(tmp_path):
    """INT32, 2%-null decimal(7,2) and dictionary strings, 300k rows in
    20k-row pages (15 page uploads per chunk), against the pyarrow read."""
    import decimal

    import pyarrow as pa
    import pyarrow.parquet as pq

    from spark_rapids_amd.io.parquet import PHASE_STATS
    from spark_rapids_amd.io.parquet_gpu import read_parquet_gpu

    n = 300_000
    rng = np.random.default_rng(7)
    i32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    cents = rng.integers(-9_999_999, 10_000_000, n)
    null = rng.integers(0, 50, n) == 0  # 2% NULL
    dec = pa.array(
        [None if z else decimal.Decimal(int(c)).scaleb(-2)
         for c, z in zip(cents, null)], pa.decimal128(7, 2))
    words = np.array([f"name-{k:04d}" for k in range(997)])
    strs = pa.array(words[rng.integers(0, len(words), n)])
    tbl = pa.table({"i": pa.array(i32), "d": dec, "s": strs})
    p = str(tmp_path / "t.parquet")
    pq.write_table(tbl, p, compression=None, use_dictionary=["s"],
                   store_decimal_as_integer=True, row_group_size=n,
                   max_rows_per_page=20_000, data_page_size=8 << 20)
    md = pq.ParquetFile(p).metadata
    assert md.num_row_groups == 1
    assert md.row_group(0).column(0).physical_type == "INT32"
    assert md.row_group(0).column(1).physical_type == "INT32"
    assert md.row_group(0).column(2).has_dictionary_page

    bytes_before = PHASE_STATS["upload_bytes"]
    batch = read_parquet_gpu(p, ["i", "d", "s"]).cpu()
    assert PHASE_STATS["upload_bytes"] - bytes_before >= 2 * 4 * n

    exp = pq.read_table(p)
    assert np.array_equal(batch.columns[0].to_numpy(), i32)
    assert batch.columns[1].to_pylist() == exp.column("d").to_pylist()
    assert batch.columns[2].to_pylist() == exp.column("s").to_pylist()
