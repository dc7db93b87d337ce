"""array_union / array_intersect / array_except / arrays_overlap (reference
analogue: GpuArrayUnion, GpuArrayIntersect, GpuArrayExcept, GpuArraysOverlap
in collectionOperations.scala).

Element equality is array_distinct's: NaN equals NaN, -0.0 equals 0.0,
strings compare by their UTF-8 bytes, a null equals a null. Whole results are
compared through repr(), so that NaN and the sign of a zero count. The GPU
tests compare a GPU session with spark.rapids.sql.enabled=False; the CPU
implementations are the oracle and are pinned by the hand-written
expectations below.
"""
import decimal
import math
import os

import numpy as np
import pytest

import spark_rapids_amd as sr  # noqa: F401
from spark_rapids_amd import Column, DType, col, collect_set
from spark_rapids_amd import ops
from spark_rapids_amd.plan.overrides import Tagger

NAN = float("nan")
INF = float("inf")
L_I64 = DType.list_(DType.int64())
L_F64 = DType.list_(DType.float64())
L_STR = DType.list_(DType.string())

A = [[1, 2, 2, None, 3], [1, None], None, [], [None, None], [4, 4]]
B = [[2, 3, 3, 5, None], [2], [1], [1], [], None]


def _four(a, b):
    return [a.array_union(b).alias("union"),
            a.array_intersect(b).alias("intersect"),
            a.array_except(b).alias("except"),
            a.arrays_overlap(b).alias("overlap")]


def _run(session, a, b, dtype):
    df = session.create_dataframe({"a": a, "b": b},
                                  dtypes={"a": dtype, "b": dtype})
    return df.select(*_four(col("a"), col("b"))).to_pydict()


# ---------------------------------------------------------------------------
# CPU: hand-written expectations
# ---------------------------------------------------------------------------

def test_base_expectations(cpu_session):
    out = _run(cpu_session, A, B, L_I64)
    assert out["union"] == [[1, 2, None, 3, 5], [1, None, 2], None, [1],
                            [None], None]
    assert out["intersect"] == [[2, None, 3], [], None, [], [], None]
    assert out["except"] == [[1], [1, None], None, [], [None], None]
    assert out["overlap"] == [True, None, None, False, False, None]


def test_float_specials(cpu_session):
    out = _run(cpu_session, [[NAN, -0.0, 1.0, NAN]], [[0.0, NAN]], L_F64)
    assert repr(out["union"]) == repr([[NAN, -0.0, 1.0]])
    assert repr(out["intersect"]) == repr([[NAN, -0.0]])
    # the surviving zero is the left operand's
    assert math.copysign(1.0, out["intersect"][0][1]) == -1.0
    assert repr(out["except"]) == repr([[1.0]])
    assert out["overlap"] == [True]


def test_overlap_null_rules(cpu_session):
    out = _run(cpu_session, [[1.0], [], [None], [1.0, None], [2.0]],
               [[None], [None], [], [1.0], [3.0]], L_F64)
    assert out["overlap"] == [None, False, False, True, False]


STR_A = [["commonprefix1", "", "é", "commonprefix", None, "a", ""],
         ["commonprefix2"], ["x", None]]
STR_B = [["commonprefix2", "commonprefix", "é", "", "b"],
         ["commonprefix1", "commonprefix"], ["y"]]


def test_strings_compare_by_bytes(cpu_session):
    out = _run(cpu_session, STR_A, STR_B, L_STR)
    assert out["union"] == [
        ["commonprefix1", "", "é", "commonprefix", None, "a",
         "commonprefix2", "b"],
        ["commonprefix2", "commonprefix1", "commonprefix"],
        ["x", None, "y"]]
    assert out["intersect"] == [["", "é", "commonprefix"], [], []]
    assert out["except"] == [["commonprefix1", None, "a"],
                             ["commonprefix2"], ["x", None]]
    assert out["overlap"] == [True, False, None]


def test_sql_functions(cpu_session):
    df = cpu_session.create_dataframe({"a": A, "b": B},
                                      dtypes={"a": L_I64, "b": L_I64})
    cpu_session.register("t", df)
    out = cpu_session.sql(
        "SELECT array_union(a, b) AS u, array_intersect(a, b) AS i, "
        "array_except(a, b) AS e, arrays_overlap(a, b) AS o "
        "FROM t").to_pydict()
    want = _run(cpu_session, A, B, L_I64)
    assert out["u"] == want["union"]
    assert out["i"] == want["intersect"]
    assert out["e"] == want["except"]
    assert out["o"] == want["overlap"]


def test_sql_argument_count(cpu_session):
    df = cpu_session.create_dataframe({"a": A, "b": B},
                                      dtypes={"a": L_I64, "b": L_I64})
    cpu_session.register("t", df)
    for q in ("array_union(a)", "arrays_overlap(a, b, a)"):
        with pytest.raises(ValueError, match="two arguments"):
            cpu_session.sql(f"SELECT {q} AS x FROM t")


def test_expression_types_and_names(cpu_session):
    df = cpu_session.create_dataframe({"a": A, "b": B},
                                      dtypes={"a": L_I64, "b": L_I64})
    a, b = col("a"), col("b")
    assert a.array_union(b).dtype(df.schema) == L_I64
    assert a.array_intersect(b).dtype(df.schema) == L_I64
    assert a.array_except(b).dtype(df.schema) == L_I64
    assert a.arrays_overlap(b).dtype(df.schema) == DType.bool_()
    assert str(a.array_union(b)) == "array_union(a, b)"
    assert str(a.array_intersect(b)) == "array_intersect(a, b)"
    assert str(a.array_except(b)) == "array_except(a, b)"
    assert str(a.arrays_overlap(b)) == "arrays_overlap(a, b)"
    assert a.array_union(b).children == (a, b)


def test_mismatched_element_types_raise(cpu_session):
    df = cpu_session.create_dataframe(
        {"a": [[1]], "b": [[1.0]], "c": [1]},
        dtypes={"a": L_I64, "b": L_F64, "c": DType.int64()})
    for other, odt in (("b", L_F64), ("c", DType.int64())):
        for e in _four(col("a"), col(other)) + _four(col(other), col("a")):
            with pytest.raises(TypeError) as ei:
                e.dtype(df.schema)
            # the message names both types
            assert str(L_I64) in str(ei.value), str(ei.value)
            assert str(odt) in str(ei.value), str(ei.value)
    with pytest.raises(TypeError):
        df.select(col("a").array_union(col("b")).alias("x")).to_pydict()


def test_tagger_element_types(session):
    def frame(data, dt):
        return session.create_dataframe({"a": data, "b": data},
                                        dtypes={"a": dt, "b": dt})

    i64 = frame(A, L_I64)
    strs = frame([["x"]], L_STR)
    d128 = frame([[decimal.Decimal("1.5"), None]],
                 DType.list_(DType.decimal(30, 2)))
    t = Tagger(session.conf)
    for e in _four(col("a"), col("b")):
        assert t.expr_reasons(e, i64.schema) == [], str(e)
        assert t.expr_reasons(e, strs.schema) == [], str(e)
        reasons = t.expr_reasons(e, d128.schema)
        assert len(reasons) == 1 and "decimal128" in reasons[0], reasons


def test_docgen_lists_set_functions(tmp_path, monkeypatch):
    from spark_rapids_amd.tools import docgen

    monkeypatch.setattr(docgen, "REPO", str(tmp_path))
    docgen.main()
    text = open(os.path.join(str(tmp_path), "docs",
                             "supported_ops.md")).read()
    rows = {ln.split("|")[1].strip(): ln.split("|")[3].strip()
            for ln in text.splitlines() if ln.startswith("| ")}
    for name in ("ArrayUnion", "ArrayIntersect", "ArrayExcept",
                 "ArraysOverlap"):
        assert rows.get(name) == "GPU", (name, rows.get(name))


def test_committed_supported_ops_is_generated(tmp_path, monkeypatch):
    """docs/supported_ops.md is docgen's output, not a hand edit."""
    from spark_rapids_amd.tools import docgen

    committed = open(os.path.join(docgen.REPO, "docs",
                                  "supported_ops.md")).read()
    monkeypatch.setattr(docgen, "REPO", str(tmp_path))
    docgen.main()
    fresh = open(os.path.join(str(tmp_path), "docs",
                              "supported_ops.md")).read()
    assert committed == fresh


# ---------------------------------------------------------------------------
# GPU vs CPU
# ---------------------------------------------------------------------------

# (len a, len b): every pair of the binary search's small sizes, the
# sub-wave -> block tier step of the sort on either side (against a short
# list and against each other), and the block -> radix tier step
_SMALL = [0, 1, 2, 3, 7, 8, 9]
_WAVE_STEP = [63, 64, 65]
_BLOCK_STEP = [2047, 2048, 2049]
LENGTH_PAIRS = (
    [(x, y) for x in _SMALL for y in _SMALL]
    + [(x, 5) for x in _WAVE_STEP] + [(5, y) for y in _WAVE_STEP]
    + [(x, y) for x in _WAVE_STEP for y in _WAVE_STEP]
    + [(x, y) for x in _BLOCK_STEP for y in (5, 300)]
    + [(x, y) for x in (5, 300) for y in _BLOCK_STEP])

_KINDS = {
    "int64": (DType.int64(), [-2 ** 63, 2 ** 63 - 1]),
    "int32": (DType.int32(), [-2 ** 31, 2 ** 31 - 1]),
    "double": (DType.float64(), [NAN, -0.0, 0.0, INF, -INF, -1.7e308,
                                 1.7e308]),
    "bool": (DType.bool_(), [True, False]),
}


def _values(kind, rng, n, spread=40):
    pool = _KINDS[kind][1]
    if kind == "bool":
        vals = [bool(v) for v in rng.integers(0, 2, n)]
    elif kind == "double":
        vals = [float(v) / 2 for v in rng.integers(-spread, spread + 1, n)]
    else:
        vals = [int(v) for v in rng.integers(-spread, spread + 1, n)]
    out = []
    for v in vals:
        r = rng.random()
        if r < 0.10:
            out.append(None)
        elif r < 0.20:
            out.append(pool[int(rng.integers(0, len(pool)))])
        else:
            out.append(v)
    return out


def _pair_rows(kind):
    """Rows of the length pairs, values from -40..40 plus the range ends
    with 10 % nulls; the long pairs once more over a range as wide as the
    lists so that they also miss; null rows on either side independently."""
    rng = np.random.default_rng(23)
    a, b = [], []
    for i, (la, lb) in enumerate(LENGTH_PAIRS):
        a.append(_values(kind, rng, la))
        b.append(_values(kind, rng, lb))
        if max(la, lb) > 65:
            a.append(_values(kind, rng, la, 2000))
            b.append(_values(kind, rng, lb, 2000))
        if i % 9 == 4:      # null on the left, a non-empty range on the right
            a.append(None)
            b.append(_values(kind, rng, 3))
        if i % 11 == 6:
            a.append(_values(kind, rng, 4))
            b.append(None)
        if i % 30 == 12:
            a.append(None)
            b.append(None)
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(_KINDS))
def test_gpu_length_pairs(kind, gpu_session, cpu_session):
    a, b = _pair_rows(kind)
    dt = DType.list_(_KINDS[kind][0])
    want = _run(cpu_session, a, b, dt)
    got = _run(gpu_session, a, b, dt)
    for name in want:
        for r, (g, w) in enumerate(zip(got[name], want[name])):
            assert repr(g) == repr(w), (kind, name, r, len(a[r] or ()),
                                        len(b[r] or ()))
        assert len(got[name]) == len(want[name])


_WORDS = ["", "a", "ab", "abc", "b", "commonprefix", "commonprefix1",
          "commonprefix2", "é", "zz", "commonprefi"]


def _short_lists(kind, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        if rng.random() < 0.05:
            rows.append(None)
            continue
        vals = []
        for _ in range(int(rng.integers(0, 13))):
            r = rng.random()
            if r < 0.1:
                vals.append(None)
            elif kind == "string":
                vals.append(_WORDS[int(rng.integers(0, len(_WORDS)))])
            elif kind == "double":
                vals.append([NAN, -0.0, 0.0, 1.5, -2.5, INF, 7.25, -INF][
                    int(rng.integers(0, 8))])
            else:
                vals.append(int(rng.integers(-6, 7)))
        rows.append(vals)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dt", [("int64", L_I64), ("double", L_F64),
                                     ("string", L_STR)])
def test_gpu_random_short_lists(kind, dt, gpu_session, cpu_session):
    a, b = _short_lists(kind, 3000, 11), _short_lists(kind, 3000, 12)
    want = _run(cpu_session, a, b, dt)
    got = _run(gpu_session, a, b, dt)
    for name in want:
        assert repr(got[name]) == repr(want[name]), (kind, name)


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [5, 8, 9, 16, 29, 32, 33, 64])
def test_gpu_overlap_lane_group_widths(max_len):
    """arrays_overlap gives the longest left row's width (8/16/32/64 lanes)
    to every row and packs 64 rows into a validity word: 203 rows are three
    full words and a partial one, the left lengths reach max_len exactly."""
    rng = np.random.default_rng(max_len)
    a, b = [], []
    for r in range(203):
        la = max_len if r == 100 else int(rng.integers(0, max_len + 1))
        a.append(None if r != 100 and rng.random() < 0.1 else
                 _values("int64", rng, la))
        b.append(None if rng.random() < 0.1 else
                 _values("int64", rng, int(rng.integers(0, 6)), 60))
    got = ops.arrays_overlap(Column.from_pylist(a, L_I64).cuda(),
                             Column.from_pylist(b, L_I64).cuda())
    want = ops.arrays_overlap(Column.from_pylist(a, L_I64),
                              Column.from_pylist(b, L_I64)).to_pylist()
    assert got.cpu().to_pylist() == want
    assert {True, False, None} <= set(want)


@pytest.mark.gpu
def test_gpu_remaining_element_types(gpu_session, cpu_session):
    """The narrower and the logical fixed-width types go through the same
    kernels with their own key transform."""
    rng = np.random.default_rng(17)
    kinds = {
        "int8": (DType.int8(), [-128, 127, 0, -1, 5, 6]),
        "int16": (DType.int16(), [-2 ** 15, 2 ** 15 - 1, 0, -1, 300, 7]),
        "float32": (DType.float32(), [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.5]),
        "date": (DType.date32(), [-1, 0, 10957, 19000, 5]),
        "timestamp": (DType.timestamp(),
                      [-1, 0, 946684800000000, 1700000000000000, 9]),
        "decimal64": (DType.decimal(12, 2),
                      [decimal.Decimal("-99.50"), decimal.Decimal("0"),
                       decimal.Decimal("12345.67"), decimal.Decimal("0.01")]),
    }
    for kind, (et, pool) in kinds.items():
        def rows():
            out = [None]
            for ln in (0, 1, 3, 5, 9, 70, 300):
                out.append([None if rng.random() < 0.1 else
                            pool[int(rng.integers(0, len(pool)))]
                            for _ in range(ln)])
            return out
        a, b = rows(), rows()[::-1]
        dt = DType.list_(et)
        want = _run(cpu_session, a, b, dt)
        got = _run(gpu_session, a, b, dt)
        for name in want:
            assert repr(got[name]) == repr(want[name]), (kind, name)


_SET_OPS = (ops.array_union, ops.array_intersect, ops.array_except,
            ops.arrays_overlap)


def _view(big, dt, lo, m):
    # word-aligned start keeps the validity view aligned
    return Column(dt, m, big.data,
                  None if big.validity is None else big.validity[lo // 8:],
                  big.offsets[lo:lo + m + 1], None, big.child)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,kind", [(L_I64, "int64"), (L_STR, "string")])
def test_gpu_nonzero_first_offsets(dt, kind):
    """Zero-copy row ranges of two larger LIST columns with different
    starts: both first offsets are non-zero and differ, and each child
    holds elements of rows outside the range."""
    ra, rb = _short_lists(kind, 400, 31), _short_lists(kind, 400, 32)
    big_a = Column.from_pylist(ra, dt).cuda()
    big_b = Column.from_pylist(rb, dt).cuda()
    m = 200
    va, vb = _view(big_a, dt, 64, m), _view(big_b, dt, 128, m)
    off_a, off_b = int(va.offsets[0].item()), int(vb.offsets[0].item())
    assert off_a > 0 and off_b > 0 and off_a != off_b
    ha = Column.from_pylist(ra[64:64 + m], dt)
    hb = Column.from_pylist(rb[128:128 + m], dt)
    before = [t.clone() for t in (big_a.offsets, big_a.child.data,
                                  big_b.offsets, big_b.child.data)]
    for fn in _SET_OPS:
        got = fn(va, vb).cpu().to_pylist()
        want = fn(ha, hb).to_pylist()
        assert repr(got) == repr(want), fn.__name__
    # inputs are never modified
    after = (big_a.offsets, big_a.child.data, big_b.offsets,
             big_b.child.data)
    for x, y in zip(before, after):
        assert bool((x == y).all())


@pytest.mark.gpu
def test_gpu_empty_inputs():
    some = [[1, None, 2], [3], [None]]
    for a, b in (([], []),
                 ([None, None, None], some), (some, [None, None, None]),
                 ([[], [], []], some), (some, [[], [], []]),
                 ([[], None, []], [None, [], []])):
        da, db = (Column.from_pylist(x, L_I64).cuda() for x in (a, b))
        ha, hb = (Column.from_pylist(x, L_I64) for x in (a, b))
        for fn in _SET_OPS:
            assert fn(da, db).cpu().to_pylist() == fn(ha, hb).to_pylist(), \
                (fn.__name__, a, b)


@pytest.mark.gpu
def test_gpu_array_distinct_unchanged_by_shared_compaction():
    """array_distinct goes through the compaction helper the set
    operations share; its result on a view with a first offset stays the
    host's."""
    rows = _short_lists("double", 400, 41)
    big = Column.from_pylist(rows, L_F64).cuda()
    got = ops.array_distinct(_view(big, L_F64, 64, 200)).cpu().to_pylist()
    want = ops.array_distinct(
        Column.from_pylist(rows[64:264], L_F64)).to_pylist()
    assert repr(got) == repr(want)


@pytest.mark.gpu
def test_gpu_plan_placement(gpu_session, cpu_session):
    for a, b, dt in ((A, B, L_I64), (STR_A, STR_B, L_STR)):
        df = gpu_session.create_dataframe({"a": a, "b": b},
                                          dtypes={"a": dt, "b": dt})
        tree = df.select(*_four(col("a"), col("b"))) \
            .physical_plan().tree_string()
        assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
    d128 = DType.list_(DType.decimal(30, 2))
    D = decimal.Decimal
    a = [[D("2.50"), None, D("-1.25"), D("2.50")], None, [], [D("1.00")]]
    b = [[D("-1.25"), D("7.00")], [D("1.00")], [None], [D("3.00"), None]]
    assert repr(_run(gpu_session, a, b, d128)) == \
        repr(_run(cpu_session, a, b, d128))


@pytest.mark.gpu
def test_gpu_set_ops_of_collect_sets(gpu_session, cpu_session):
    rng = np.random.default_rng(3)
    n = 5000
    data = {"k": [int(v) for v in rng.integers(0, 40, n)],
            "x": [None if v == 7 else int(v)
                  for v in rng.integers(0, 25, n)],
            "y": [int(v) for v in rng.integers(10, 40, n)]}

    def q(s):
        df = s.create_dataframe(data)
        xs, ys = col("xs"), col("ys")
        rows = (df.group_by("k")
                .agg(collect_set(col("x")).alias("xs"),
                     collect_set(col("y")).alias("ys"))
                .select(col("k"),
                        xs.array_intersect(ys).sort_array().alias("i"),
                        xs.array_union(ys).sort_array().alias("u"),
                        xs.array_except(ys).sort_array().alias("e"),
                        xs.arrays_overlap(ys).alias("o"))
                .collect())
        return sorted(rows)

    got, want = q(gpu_session), q(cpu_session)
    assert got == want
    assert any(r[1] for r in want) and any(r[3] for r in want)
