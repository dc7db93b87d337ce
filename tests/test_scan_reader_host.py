"""The parquet page walker of the native scan reader
(native/hipdf/kernels/pq_pieces.h), run on the host under the sanitizers as a
stand-alone program. The column chunks are cut out of files that pyarrow
writes here."""
import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "native", "hipdf")

_WIDTH = {"INT32": 4, "INT64": 8, "FLOAT": 4, "DOUBLE": 8}
_TYPES = [("INT32", pa.int32(), np.int32), ("INT64", pa.int64(), np.int64),
          ("DOUBLE", pa.float64(), np.float64)]


@pytest.fixture(scope="module")
def pieces_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pp") / "pq_pieces_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall",
                    "-fsanitize=address,undefined",
                    "-I" + os.path.join(NATIVE, "kernels"),
                    os.path.join(NATIVE, "tests", "pq_pieces_host_test.cpp"),
                    "-o", exe], check=True)
    return exe


def _values(np_dt, n):
    rng = np.random.default_rng(n + np.dtype(np_dt).itemsize)
    if np.issubdtype(np_dt, np.floating):
        return rng.standard_normal(n).astype(np_dt)
    info = np.iinfo(np_dt)
    v = rng.integers(info.min, info.max, n, dtype=np_dt, endpoint=True)
    if n >= 2:
        v[0], v[1] = info.min, info.max
    return v


def _write_chunk(tmp, name, array, nullable, **opts):
    """Write a one-column file; returns (chunk file, num_values, max_def,
    physical width) of its only column chunk."""
    schema = pa.schema([pa.field("c", array.type, nullable=nullable)])
    path = os.path.join(tmp, name + ".parquet")
    kw = dict(compression=None, use_dictionary=False)
    kw.update(opts)
    pq.write_table(pa.table({"c": array}, schema=schema), path, **kw)
    pf = pq.ParquetFile(path)
    md = pf.metadata
    chunk_path = os.path.join(tmp, name + ".chunk")
    if md.num_row_groups == 0:
        open(chunk_path, "wb").close()
        return chunk_path, 0, pf.schema.column(0).max_definition_level, \
            _WIDTH.get(str(pf.schema.column(0).physical_type), 0)
    assert md.num_row_groups == 1
    cmd = md.row_group(0).column(0)
    start = cmd.dictionary_page_offset \
        if cmd.has_dictionary_page else cmd.data_page_offset
    with open(path, "rb") as f:
        f.seek(start)
        raw = f.read(cmd.total_compressed_size)
    with open(chunk_path, "wb") as f:
        f.write(raw)
    return chunk_path, cmd.num_values, \
        pf.schema.column(0).max_definition_level, \
        _WIDTH.get(cmd.physical_type, 0)


def _run(exe, tmp, lines):
    cases = os.path.join(tmp, "cases.txt")
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout


def test_eligible_chunks_give_their_values(pieces_exe, tmp_path):
    tmp = str(tmp_path)
    lines = []
    for phys, pa_t, np_dt in _TYPES:
        for nullable in (False, True):
            for version in ("1.0", "2.0"):
                for rows, pages in ((1000, 1), (5000, 5), (0, None)):
                    vals = _values(np_dt, rows)
                    name = f"{phys}_{int(nullable)}_{version[0]}_{rows}"
                    chunk, n, max_def, width = _write_chunk(
                        tmp, name, pa.array(vals, type=pa_t), nullable,
                        data_page_version=version, max_rows_per_page=1000,
                        # far above 1000 rows: the row cap alone cuts pages
                        data_page_size=1 << 20)
                    assert n == rows and width == _WIDTH[phys]
                    assert max_def == int(nullable)
                    want = os.path.join(tmp, name + ".values")
                    vals.astype(vals.dtype.newbyteorder("<")).tofile(want)
                    if pages is None:
                        # an empty chunk is no page or one page of 0 values
                        pages = 1 if os.path.getsize(chunk) else 0
                    lines.append(f"{chunk} {n} {max_def} {width} ok {pages} "
                                 f"{want}")
    out = _run(pieces_exe, tmp, lines)
    assert f"cases {len(lines)} " in out and len(lines) == 36


def test_ineligible_chunks_are_rejected(pieces_exe, tmp_path):
    tmp = str(tmp_path)
    n = 3000
    ints = (np.arange(n) % 50).astype(np.int32)
    mask = np.zeros(n, dtype=bool)
    mask[::50] = True  # 2% nulls
    lines = []
    for version in ("1.0", "2.0"):
        v = version[0]
        cases = [
            ("nulls" + v, pa.array(ints, mask=mask), True, {}),
            ("dict" + v, pa.array(ints), False, {"use_dictionary": True}),
            ("snappy" + v, pa.array(ints), False, {"compression": "snappy"}),
            ("bytes" + v, pa.array([f"s{i % 7}" for i in range(n)]), False,
             {}),
        ]
        for name, arr, nullable, opts in cases:
            chunk, nv, max_def, width = _write_chunk(
                tmp, name, arr, nullable, data_page_version=version, **opts)
            assert nv == n
            lines.append(f"{chunk} {nv} {max_def} {width} err")
            if name.startswith("bytes"):
                # BYTE_ARRAY is refused by its width; it must also not walk
                # when a caller claims a fixed width for it
                assert width == 0
                lines.append(f"{chunk} {nv} {max_def} 4 err")
    out = _run(pieces_exe, tmp, lines)
    assert f"cases {len(lines)} " in out and len(lines) == 10


def test_every_truncated_prefix_is_an_error(pieces_exe, tmp_path):
    tmp = str(tmp_path)
    lines = []
    for version, nullable in (("1.0", True), ("2.0", True), ("1.0", False)):
        vals = _values(np.int32, 60)
        chunk, n, max_def, width = _write_chunk(
            tmp, f"small{version[0]}{int(nullable)}",
            pa.array(vals, type=pa.int32()), nullable,
            data_page_version=version, max_rows_per_page=20,
            data_page_size=1 << 20)
        lines.append(f"{chunk} {n} {max_def} {width} trunc")
    out = _run(pieces_exe, tmp, lines)
    assert "cases 3 " in out and "prefixes 0 " not in out
