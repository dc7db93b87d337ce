"""sort_array / array_sort / array_distinct / array_min / array_max
(reference analogue: GpuSortArray, GpuArraySort, GpuArrayDistinct
KEEP_FIRST, GpuArrayMin/Max in collectionOperations.scala).

Results hold floats, so whole results are compared through repr(): every
NaN prints alike and -0.0 prints apart from 0.0, which == does not give.
The GPU tests compare a GPU session with spark.rapids.sql.enabled=False;
the CPU implementations are the oracle and are pinned by the hand-written
expectations below.
"""
import decimal
import math
import os

import numpy as np
import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, DType, col, collect_set
from spark_rapids_amd import ops
from spark_rapids_amd.plan.overrides import Tagger

NAN = float("nan")
INF = float("inf")
BASE = [[3, None, 1, 2], [], None, [None, None], [5]]
FLOATS = [NAN, 1.0, -0.0, 0.0, -INF, None, NAN]
L_I64 = DType.list_(DType.int64())
L_F64 = DType.list_(DType.float64())
L_STR = DType.list_(DType.string())


def _five(c):
    """The six projections every test runs: both sort directions,
    array_sort, distinct, min, max."""
    return [c.sort_array().alias("asc"),
            c.sort_array(False).alias("desc"),
            c.array_sort().alias("asort"),
            c.array_distinct().alias("dist"),
            c.array_min().alias("mn"),
            c.array_max().alias("mx")]


def _run(session, data, dtype):
    df = session.create_dataframe({"a": data}, dtypes={"a": dtype})
    return df.select(*_five(col("a"))).to_pydict()


# ---------------------------------------------------------------------------
# CPU: hand-written expectations
# ---------------------------------------------------------------------------

def test_base_expectations(cpu_session):
    out = _run(cpu_session, BASE, L_I64)
    assert out["asc"] == [[None, 1, 2, 3], [], None, [None, None], [5]]
    assert out["desc"] == [[3, 2, 1, None], [], None, [None, None], [5]]
    assert out["asort"] == [[1, 2, 3, None], [], None, [None, None], [5]]
    assert out["dist"] == [[3, None, 1, 2], [], None, [None], [5]]
    assert out["mn"] == [1, None, None, None, 5]
    assert out["mx"] == [3, None, None, None, 5]


def test_distinct_keeps_first_occurrence(cpu_session):
    data = [[2, None, 1, 2, None, 1, 3]]
    out = _run(cpu_session, data, L_I64)
    assert out["dist"] == [[2, None, 1, 3]]


def test_float_specials_stable_and_bit_exact(cpu_session):
    out = _run(cpu_session, [FLOATS], L_F64)
    # stable: -0.0 stays before 0.0 in both directions, NaN is greatest,
    # ascending nulls first / descending nulls last
    assert repr(out["asc"]) == repr([[None, -INF, -0.0, 0.0, 1.0, NAN, NAN]])
    assert repr(out["desc"]) == repr([[NAN, NAN, 1.0, -0.0, 0.0, -INF, None]])
    assert repr(out["asort"]) == repr([[-INF, -0.0, 0.0, 1.0, NAN, NAN, None]])
    # NaN == NaN and -0.0 == 0.0 for distinct; the first one survives
    assert repr(out["dist"]) == repr([[NAN, 1.0, -0.0, -INF, None]])
    assert out["mn"] == [-INF]
    assert math.isnan(out["mx"][0])
    assert math.copysign(1.0, out["asc"][0][2]) == -1.0
    assert math.copysign(1.0, out["asc"][0][3]) == 1.0


def test_min_is_nan_only_when_all_nan(cpu_session):
    out = _run(cpu_session, [[NAN, None, NAN], [NAN, 2.0], [0.0, -0.0]],
               L_F64)
    assert repr(out["mn"]) == repr([NAN, 2.0, 0.0])
    assert repr(out["mx"]) == repr([NAN, NAN, 0.0])
    assert repr(out["dist"]) == repr([[NAN, None], [NAN, 2.0], [0.0]])


def test_strings_order_by_utf8_bytes(cpu_session):
    data = [["b", "", None, "ab", "a", "abc", "é", "a"], None, []]
    out = _run(cpu_session, data, L_STR)
    assert out["asc"] == [[None, "", "a", "a", "ab", "abc", "b", "é"],
                          None, []]
    assert out["desc"] == [["é", "b", "abc", "ab", "a", "a", "", None],
                           None, []]
    assert out["dist"] == [["b", "", None, "ab", "a", "abc", "é"], None, []]
    assert out["mn"] == ["", None, None]
    assert out["mx"] == ["é", None, None]


def test_sql_functions(cpu_session):
    df = cpu_session.create_dataframe({"a": BASE}, dtypes={"a": L_I64})
    cpu_session.register("t", df)
    out = cpu_session.sql(
        "SELECT sort_array(a) AS s0, sort_array(a, true) AS s1, "
        "sort_array(a, false) AS s2, array_sort(a) AS s3, "
        "array_distinct(a) AS s4, array_min(a) AS s5, array_max(a) AS s6 "
        "FROM t").to_pydict()
    want = _run(cpu_session, BASE, L_I64)
    assert out["s0"] == want["asc"] and out["s1"] == want["asc"]
    assert out["s2"] == want["desc"]
    assert out["s3"] == want["asort"]
    assert out["s4"] == want["dist"]
    assert out["s5"] == want["mn"] and out["s6"] == want["mx"]


def test_sql_float_case(cpu_session):
    df = cpu_session.create_dataframe({"a": [FLOATS]}, dtypes={"a": L_F64})
    cpu_session.register("f", df)
    out = cpu_session.sql(
        "SELECT sort_array(a, false) AS d, array_distinct(a) AS u "
        "FROM f").to_pydict()
    assert repr(out["d"]) == repr([[NAN, NAN, 1.0, -0.0, 0.0, -INF, None]])
    assert repr(out["u"]) == repr([[NAN, 1.0, -0.0, -INF, None]])


def test_expression_types_and_names(cpu_session):
    df = cpu_session.create_dataframe({"a": BASE}, dtypes={"a": L_I64})
    c = col("a")
    assert c.sort_array(False).dtype(df.schema) == L_I64
    assert c.array_distinct().dtype(df.schema) == L_I64
    assert c.array_sort().dtype(df.schema) == L_I64
    assert c.array_min().dtype(df.schema) == DType.int64()
    assert c.array_max().dtype(df.schema) == DType.int64()
    assert str(c.sort_array(False)) == "sort_array(a, false)"
    assert str(c.array_sort()) == "array_sort(a)"
    assert str(c.array_max()) == "array_max(a)"


def test_tagger_element_types(session):
    i64 = session.create_dataframe({"a": BASE}, dtypes={"a": L_I64})
    d128 = session.create_dataframe(
        {"a": [[decimal.Decimal("1.5"), None]]},
        dtypes={"a": DType.list_(DType.decimal(30, 2))})
    strs = session.create_dataframe({"a": [["x"]]}, dtypes={"a": L_STR})
    t = Tagger(session.conf)
    for e in _five(col("a")):
        assert t.expr_reasons(e, i64.schema) == [], str(e)
        assert t.expr_reasons(e, strs.schema) == [], str(e)
        reasons = t.expr_reasons(e, d128.schema)
        assert len(reasons) == 1 and "decimal128" in reasons[0], reasons


def test_docgen_lists_array_functions(tmp_path, monkeypatch):
    from spark_rapids_amd.tools import docgen

    monkeypatch.setattr(docgen, "REPO", str(tmp_path))
    docgen.main()
    text = open(os.path.join(str(tmp_path), "docs",
                             "supported_ops.md")).read()
    rows = {ln.split("|")[1].strip(): ln.split("|")[3].strip()
            for ln in text.splitlines() if ln.startswith("| ")}
    for name in ("SortArray", "ArraySort", "ArrayDistinct", "ArrayMin",
                 "ArrayMax"):
        assert rows.get(name) == "GPU", (name, rows.get(name))


# ---------------------------------------------------------------------------
# GPU vs CPU
# ---------------------------------------------------------------------------

# every tier boundary: the W = 8/16/32/64 lane groups, the 64 -> block tier
# step, powers of two inside the block tier, its 2048 cap, and the long tier
LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256,
           257, 2047, 2048, 2049, 5000]

_KINDS = {
    "int64": DType.int64(), "int32": DType.int32(),
    "double": DType.float64(), "bool": DType.bool_(),
}


def _values(kind, rng, n):
    if kind == "int64":
        pool = [-2 ** 63, 2 ** 63 - 1, 0, -1, 1]
        vals = [int(v) for v in rng.integers(-40, 40, n)]
    elif kind == "int32":
        pool = [-2 ** 31, 2 ** 31 - 1, 0]
        vals = [int(v) for v in rng.integers(-40, 40, n)]
    elif kind == "double":
        pool = [NAN, -0.0, 0.0, INF, -INF, 1e-300, -1e300]
        vals = [float(v) for v in np.round(rng.normal(0, 3, n), 1)]
    else:
        pool = [True, False]
        vals = [bool(v) for v in rng.integers(0, 2, n)]
    out = []
    for v in vals:
        r = rng.random()
        if r < 0.10:
            out.append(None)
        elif r < 0.25:
            out.append(pool[int(rng.integers(0, len(pool)))])
        else:
            out.append(v)
    return out


def _boundary_rows(kind, max_len):
    rng = np.random.default_rng(7)
    rows = []
    for ln in LENGTHS:
        if ln > max_len:
            continue
        rows.append(_values(kind, rng, ln))
        if ln in (2, 16, 65, 2048):
            rows.append(None)  # null rows between the tiers
    rows.append(None)
    rows.append([None, None, None])
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [8, 16, 32, 64, 5000])
@pytest.mark.parametrize("kind", list(_KINDS))
def test_gpu_boundary_lengths(kind, max_len, gpu_session, cpu_session):
    rows = _boundary_rows(kind, max_len)
    dt = DType.list_(_KINDS[kind])
    want = _run(cpu_session, rows, dt)
    got = _run(gpu_session, rows, dt)
    for name in want:
        assert repr(got[name]) == repr(want[name]), (kind, max_len, name)


@pytest.mark.gpu
def test_gpu_remaining_element_types(gpu_session, cpu_session):
    """The narrower and the logical fixed-width types go through the same
    kernels with their own key transform: lists in the sub-wave and block
    tiers, values at both ends of each range."""
    rng = np.random.default_rng(17)
    dec = DType.decimal(12, 2)
    kinds = {
        "int8": (DType.int8(), [-128, 127, 0, -1, 5]),
        "int16": (DType.int16(), [-2 ** 15, 2 ** 15 - 1, 0, -1, 300]),
        "float32": (DType.float32(), [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.5]),
        "date": (DType.date32(), [-1, 0, 10957, 19000]),
        "timestamp": (DType.timestamp(),
                      [-1, 0, 946684800000000, 1700000000000000]),
        "decimal64": (dec, [decimal.Decimal("-99.50"), decimal.Decimal("0"),
                            decimal.Decimal("12345.67")]),
    }
    for kind, (et, pool) in kinds.items():
        rows = [None]
        for ln in (0, 1, 5, 9, 70, 300):
            rows.append([None if rng.random() < 0.1 else
                         pool[int(rng.integers(0, len(pool)))]
                         for _ in range(ln)])
        dt = DType.list_(et)
        want = _run(cpu_session, rows, dt)
        got = _run(gpu_session, rows, dt)
        for name in want:
            assert repr(got[name]) == repr(want[name]), (kind, name)


def _short_lists(kind, n=3000):
    rng = np.random.default_rng(11)
    words = ["", "a", "ab", "abc", "b", "commonprefix", "commonprefix1",
             "commonprefix2", "é", "zz"]
    rows = []
    for _ in range(n):
        if rng.random() < 0.05:
            rows.append(None)
            continue
        ln = int(rng.integers(0, 13))
        vals = []
        for _ in range(ln):
            r = rng.random()
            if r < 0.1:
                vals.append(None)
            elif kind == "string":
                vals.append(words[int(rng.integers(0, len(words)))])
            elif kind == "double":
                vals.append([NAN, -0.0, 0.0, 1.5, -2.5, INF][
                    int(rng.integers(0, 6))])
            else:
                vals.append(int(rng.integers(-4, 5)))
        rows.append(vals)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dt", [("int64", L_I64), ("double", L_F64),
                                     ("string", L_STR)])
def test_gpu_random_short_lists(kind, dt, gpu_session, cpu_session):
    rows = _short_lists(kind)
    want = _run(cpu_session, rows, dt)
    got = _run(gpu_session, rows, dt)
    for name in want:
        assert repr(got[name]) == repr(want[name]), (kind, name)


@pytest.mark.gpu
def test_gpu_string_lists_past_the_wave_tier(gpu_session, cpu_session):
    rng = np.random.default_rng(5)
    rows = [[None if rng.random() < 0.1 else
             "k%d" % int(rng.integers(0, 50)) * int(rng.integers(1, 4))
             for _ in range(ln)] for ln in (65, 300, 2049)]
    want = _run(cpu_session, rows, L_STR)
    got = _run(gpu_session, rows, L_STR)
    for name in want:
        assert got[name] == want[name], name


@pytest.mark.gpu
@pytest.mark.parametrize("dt,kind", [(L_I64, "int64"), (L_STR, "string")])
def test_gpu_nonzero_first_offset(dt, kind):
    """A zero-copy row range of a larger LIST column: offsets start past
    0 and the child holds elements of rows outside the range, which must
    not show up in any result."""
    rows = _short_lists(kind, 400)
    big = Column.from_pylist(rows, dt).cuda()
    lo, m = 64, 200  # word-aligned start keeps the validity view aligned
    view = Column(dt, m, big.data,
                  None if big.validity is None else big.validity[lo // 8:],
                  big.offsets[lo:lo + m + 1], None, big.child)
    assert int(view.offsets[0].item()) > 0
    host = Column.from_pylist(rows[lo:lo + m], dt)
    before = (big.offsets.clone(), big.child.data.clone())
    for fn, args in ((ops.sort_array, (True, True)),
                     (ops.sort_array, (False, False)),
                     (ops.sort_array, (True, False)),
                     (ops.array_distinct, ()), (ops.array_min, ()),
                     (ops.array_max, ())):
        got = fn(view, *args).cpu().to_pylist()
        want = fn(host, *args).to_pylist()
        assert repr(got) == repr(want), (fn.__name__, args)
    # inputs are never modified
    assert bool((before[0] == big.offsets).all())
    assert bool((before[1] == big.child.data).all())


@pytest.mark.gpu
def test_gpu_empty_inputs():
    for rows in ([], [[], None, []], [None]):
        dev = Column.from_pylist(rows, L_I64).cuda()
        host = Column.from_pylist(rows, L_I64)
        for fn in (ops.sort_array, ops.array_distinct, ops.array_min,
                   ops.array_max):
            assert fn(dev).cpu().to_pylist() == fn(host).to_pylist()


@pytest.mark.gpu
def test_gpu_plan_placement(gpu_session, cpu_session):
    for data, dt in ((BASE, L_I64), ([["b", None, "a"], None], L_STR)):
        df = gpu_session.create_dataframe({"a": data}, dtypes={"a": dt})
        tree = df.select(*_five(col("a"))).physical_plan().tree_string()
        assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
    d128 = DType.list_(DType.decimal(30, 2))
    data = [[decimal.Decimal("2.50"), None, decimal.Decimal("-1.25"),
             decimal.Decimal("2.50")], None, []]
    assert repr(_run(gpu_session, data, d128)) == \
        repr(_run(cpu_session, data, d128))


@pytest.mark.gpu
def test_gpu_sort_array_of_collect_set(gpu_session, cpu_session):
    rng = np.random.default_rng(3)
    n = 5000
    data = {"k": [int(v) for v in rng.integers(0, 40, n)],
            "x": [None if v == 7 else int(v)
                  for v in rng.integers(0, 25, n)]}

    def q(s):
        df = s.create_dataframe(data)
        rows = (df.group_by("k").agg(collect_set(col("x")).alias("xs"))
                .select(col("k"), col("xs").sort_array().alias("s"),
                        col("xs").sort_array(False).alias("d"),
                        col("xs").array_max().alias("mx"))
                .collect())
        return sorted(rows)

    assert q(gpu_session) == q(cpu_session)
