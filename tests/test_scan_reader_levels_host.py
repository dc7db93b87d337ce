"""The nullable page walk and the definition-level decoder of the native scan
reader (native/hipdf/kernels/pq_levels.h), run on the host under the
sanitizers as a stand-alone program. The column chunks are cut out of files
that pyarrow writes here; the hand-built level streams are written byte by
byte."""
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
PAGE = 1000


@pytest.fixture(scope="module")
def levels_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pl") / "pq_levels_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall",
                    "-fsanitize=address,undefined",
                    "-I" + os.path.join(NATIVE, "kernels"),
                    os.path.join(NATIVE, "tests", "pq_levels_host_test.cpp"),
                    "-o", exe], check=True)
    return exe


def _values(np_dt, n):
    rng = np.random.default_rng(n + np.dtype(np_dt).itemsize)
    if np.issubdtype(np_dt, np.floating):
        return rng.standard_normal(n).astype(np_dt)
    info = np.iinfo(np_dt)
    return rng.integers(info.min, info.max, n, dtype=np_dt, endpoint=True)


def _null_mask(pattern: str, n: int) -> np.ndarray:
    """True = NULL."""
    m = np.zeros(n, dtype=bool)
    if pattern == "random2":
        m = np.random.default_rng(n).random(n) < 0.02
    elif pattern == "all":
        m[:] = True
    elif pattern == "none":
        pass
    elif pattern == "edges":  # first and last row of every page
        m[0::PAGE] = True
        m[PAGE - 1::PAGE] = True
        if n:
            m[n - 1] = True
    elif pattern == "alternating":
        m[0::2] = True
    elif pattern == "run100":  # 100 nulls inside 1000 valid rows
        m[min(450, n):min(550, n)] = True
    else:
        raise AssertionError(pattern)
    return m


_PATTERNS = ["random2", "all", "none", "edges", "alternating", "run100"]


def _write_chunk(tmp, name, array, **opts):
    """Write a one-column nullable file; returns (chunk file, num_values,
    max_def, physical width) of its only column chunk."""
    schema = pa.schema([pa.field("c", array.type, nullable=True)])
    path = os.path.join(tmp, name + ".parquet")
    kw = dict(compression=None, use_dictionary=False,
              max_rows_per_page=PAGE, data_page_size=1 << 20)
    kw.update(opts)
    pq.write_table(pa.table({"c": array}, schema=schema), path, **kw)
    pf = pq.ParquetFile(path)
    md = pf.metadata
    chunk_path = os.path.join(tmp, name + ".chunk")
    sc = pf.schema.column(0)
    if md.num_row_groups == 0:
        open(chunk_path, "wb").close()
        return chunk_path, 0, sc.max_definition_level, \
            _WIDTH[str(sc.physical_type)]
    assert md.num_row_groups == 1
    cmd = md.row_group(0).column(0)
    assert not cmd.has_dictionary_page
    with open(path, "rb") as f:
        f.seek(cmd.data_page_offset)
        raw = f.read(cmd.total_compressed_size)
    with open(chunk_path, "wb") as f:
        f.write(raw)
    # check the matrix against pyarrow's own read of the file
    assert pq.read_table(path)["c"].null_count == array.null_count
    return chunk_path, cmd.num_values, sc.max_definition_level, \
        _WIDTH[cmd.physical_type]


def _run(exe, tmp, lines):
    cases = os.path.join(tmp, "cases.txt")
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_pages_decode_to_pyarrows_validity(levels_exe, tmp_path, version):
    tmp = str(tmp_path)
    lines = []
    pages_total = 0
    for phys, pa_t, np_dt in _TYPES:
        for rows in (0, 1, 7, 8, 9, 1000, 5000):
            for pattern in _PATTERNS:
                vals = _values(np_dt, rows)
                null = _null_mask(pattern, rows)
                arr = pa.array(vals, type=pa_t, mask=null)
                name = f"{phys}_{version[0]}_{rows}_{pattern}"
                chunk, n, max_def, width = _write_chunk(
                    tmp, name, arr, data_page_version=version)
                assert n == rows and max_def == 1 and width == _WIDTH[phys]
                # what the decode must give is pyarrow's is_null of the array
                valid = ~np.asarray(arr.is_null())
                vpath = os.path.join(tmp, name + ".valid")
                valid.astype(np.uint8).tofile(vpath)
                dpath = os.path.join(tmp, name + ".values")
                vals[valid].astype(vals.dtype.newbyteorder("<")).tofile(dpath)
                pages = (rows + PAGE - 1) // PAGE
                if rows == 0:
                    # an empty chunk is no page or one page of 0 values
                    pages = 1 if os.path.getsize(chunk) else 0
                pages_total += pages
                lines.append(f"chunk {chunk} {n} {max_def} {width} {pages} "
                             f"{vpath} {dpath}")
    out = _run(levels_exe, tmp, lines)
    assert len(lines) == 3 * 7 * 6
    assert f"cases {len(lines)} pages {pages_total} " in out


def _varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _rle(count: int, value: int) -> bytes:
    return _varint(count << 1) + bytes([value])


def _packed(groups: int, data: bytes) -> bytes:
    return _varint(groups << 1 | 1) + data


def test_hand_built_streams(levels_exe, tmp_path):
    tmp = str(tmp_path)
    lines = []

    def case(name, stream, n, want):
        p = os.path.join(tmp, name + ".lv")
        with open(p, "wb") as f:
            f.write(stream)
        if want is None:
            lines.append(f"stream {p} {n} err")
            return
        want = np.asarray(want, dtype=np.uint8)
        assert len(want) == n
        v = os.path.join(tmp, name + ".valid")
        want.tofile(v)
        lines.append(f"stream {p} {n} ok {v}")

    # an RLE run longer than the rows left is clamped
    case("rle_long", _rle(1000, 1), 10, [1] * 10)
    case("rle_long0", _rle(3, 1) + _rle(1 << 40, 0), 11, [1] * 3 + [0] * 8)
    # bit-packed padding beyond n is ignored, set bits included
    case("pad", _packed(1, b"\xff"), 5, [1] * 5)
    case("pad2", _packed(2, b"\x55\xff"), 11,
         [1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1])
    # a bit-packed run that announces more groups than the rows need
    case("groups_long", _packed(100, b"\x0f"), 4, [1] * 4)
    # runs need not start on a multiple of 8 rows
    case("unaligned", _rle(3, 1) + _packed(2, b"\xa5\x0f") + _rle(5, 0)
         + _packed(1, b"\xff") + _rle(2, 1),
         3 + 16 + 5 + 8 + 2,
         [1] * 3 + [1, 0, 1, 0, 0, 1, 0, 1] + [1, 1, 1, 1, 0, 0, 0, 0]
         + [0] * 5 + [1] * 8 + [1] * 2)
    # across a tile of 2048 rows, unaligned
    case("tiles", _rle(2045, 1) + _packed(1, b"\x5a") + _rle(3000, 1), 5000,
         [1] * 2045 + [0, 1, 0, 1, 1, 0, 1, 0] + [1] * 2947)
    case("empty", b"", 0, [])
    # errors
    case("zero_rle", _rle(0, 1) + _rle(8, 1), 8, None)
    case("zero_packed", _packed(0, b"") + _rle(8, 1), 8, None)
    case("value2", _rle(8, 2), 8, None)
    case("value2_late", _rle(4, 1) + _rle(4, 2), 8, None)
    case("short", _rle(4, 1), 8, None)
    case("short_packed", _packed(2, b"\xff"), 16, None)
    case("no_value", _varint(8 << 1), 8, None)
    case("long_varint", b"\x80" * 11 + b"\x01", 8, None)
    out = _run(levels_exe, tmp, lines)
    assert f"cases {len(lines)} " in out and len(lines) == 16


def test_every_truncated_prefix_is_an_error(levels_exe, tmp_path):
    tmp = str(tmp_path)
    lines = []
    for version in ("1.0", "2.0"):
        for pattern in ("random2", "alternating", "run100"):
            rows = 2100
            vals = _values(np.int32, rows)
            arr = pa.array(vals, type=pa.int32(),
                           mask=_null_mask(pattern, rows))
            chunk, n, max_def, width = _write_chunk(
                tmp, f"t{version[0]}_{pattern}", arr,
                data_page_version=version)
            lines.append(f"chunktrunc {chunk} {n} {max_def} {width}")
    out = _run(levels_exe, tmp, lines)
    assert "cases 6 " in out and "prefixes 0 " not in out
