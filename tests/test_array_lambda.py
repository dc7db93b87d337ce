"""transform / filter / exists / forall over arrays with lambdas (reference
analogue: GpuArrayTransform, GpuArrayFilter, GpuArrayExists in
higherOrderFunctions.scala).

The lambda body is evaluated as an ordinary projection over the flattened
child; the device side adds the element-to-row map (list_elem_rows) and the
three-valued per-row reduction (list_bool_reduce). Whole results are compared
through repr(), so that NaN and the sign of a zero count. The GPU tests
compare a GPU session with spark.rapids.sql.enabled=False, or the ops on
.cuda() columns with the ops on host columns; the CPU implementations are the
oracle and are pinned by the hand-written expectations below.
"""
import decimal
import os

import numpy as np
import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import (Column, ColumnBatch, DType, Field, Schema, col,
                              exists, filter_, forall, lit, ops,
                              substring_index, transform)
from spark_rapids_amd.expr.expressions import (ArrayExists, ArrayFilter,
                                               ArrayForAll, ArrayTransform,
                                               LambdaFunction, LambdaVariable)
from spark_rapids_amd.plan.optimizer import _expr_refs
from spark_rapids_amd.plan.overrides import Tagger

NAN = float("nan")
I64 = DType.int64()
L_I64 = DType.list_(DType.int64())
L_F64 = DType.list_(DType.float64())
L_STR = DType.list_(DType.string())

A = [[1, 2, None, 3], [], None, [None], [4, -4]]
K = [10, 20, 30, 40, 50]

# (DSL expression, SQL text, expected) over A and K
BASE = [
    (lambda a: a.transform(lambda x: x * 2), "transform(a, x -> x * 2)",
     [[2, 4, None, 6], [], None, [None], [8, -8]]),
    (lambda a: a.transform(lambda x, i: x + i),
     "transform(a, (x, i) -> x + i)",
     [[1, 3, None, 6], [], None, [None], [4, -3]]),
    (lambda a: a.transform(lambda x: x + col("k")),
     "transform(a, x -> x + k)",
     [[11, 12, None, 13], [], None, [None], [54, 46]]),
    (lambda a: a.filter(lambda x: x > 1), "filter(a, x -> x > 1)",
     [[2, 3], [], None, [], [4]]),
    (lambda a: a.filter(lambda x, i: i >= 1), "filter(a, (x, i) -> i >= 1)",
     [[2, None, 3], [], None, [], [-4]]),
    (lambda a: a.exists(lambda x: x > 2), "exists(a, x -> x > 2)",
     [True, False, None, None, True]),
    (lambda a: a.exists(lambda x: x > 5), "exists(a, x -> x > 5)",
     [None, False, None, None, False]),
    (lambda a: a.forall(lambda x: x > 0), "forall(a, x -> x > 0)",
     [None, True, None, None, False]),
    (lambda a: a.forall(lambda x: x.is_null() | (x > 0)),
     "forall(a, x -> x IS NULL OR x > 0)",
     [True, True, None, True, False]),
]


def _base_frame(session):
    return session.create_dataframe({"a": A, "k": K},
                                    dtypes={"a": L_I64, "k": I64})


def _one(df, e):
    return df.select(e.alias("r")).to_pydict()["r"]


# ---------------------------------------------------------------------------
# CPU: hand-written expectations
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(BASE)))
def test_base_expectations(case, cpu_session):
    build, _, want = BASE[case]
    assert _one(_base_frame(cpu_session), build(col("a"))) == want


@pytest.mark.parametrize("case", range(len(BASE)))
def test_sql_matches_dsl(case, cpu_session):
    _, text, want = BASE[case]
    cpu_session.register("t", _base_frame(cpu_session))
    out = cpu_session.sql(f"SELECT {text} AS r FROM t").to_pydict()
    assert out["r"] == want


def test_module_level_functions(cpu_session):
    df = _base_frame(cpu_session)
    assert _one(df, transform(col("a"), lambda x: x * 2)) == BASE[0][2]
    assert _one(df, filter_(col("a"), lambda x: x > 1)) == BASE[3][2]
    assert _one(df, exists(col("a"), lambda x: x > 2)) == BASE[5][2]
    assert _one(df, forall(col("a"), lambda x: x > 0)) == BASE[7][2]
    for name in ("transform", "filter_", "exists", "forall"):
        assert hasattr(sr, name)


def test_cpu_element_rows():
    c = Column.from_pylist(A, L_I64)
    rowid, pos = ops.list_element_rows(c)
    assert rowid.to_pylist() == [0, 0, 0, 0, 3, 4, 4]
    assert pos.to_pylist() == [0, 1, 2, 3, 0, 0, 1]
    assert rowid.dtype == DType.int32() and pos.dtype == DType.int32()
    rowid, pos = ops.list_element_rows(c, with_pos=False)
    assert rowid.to_pylist() == [0, 0, 0, 0, 3, 4, 4] and pos is None
    assert ops.list_span(c) == (0, 7)


def test_cpu_predicate_ops():
    c = Column.from_pylist(A, L_I64)
    pred = Column.from_pylist([True, False, None, True, None, False, False],
                              DType.bool_())
    assert ops.array_filter(c, pred).to_pylist() == \
        [[1, 3], [], None, [], []]
    assert ops.array_exists(c, pred).to_pylist() == \
        [True, False, None, None, False]
    assert ops.array_forall(c, pred).to_pylist() == \
        [False, True, None, None, False]
    with pytest.raises(ValueError):
        ops.array_filter(c, Column.from_pylist([True], DType.bool_()))


def test_transform_may_change_the_type(cpu_session):
    df = cpu_session.create_dataframe(
        {"s": [["ab", None, ""], None, ["xyz"]]}, dtypes={"s": L_STR})
    e = col("s").transform(lambda x: x.length())
    assert e.dtype(df.schema) == DType.list_(DType.int32())
    out = df.select(e.alias("r"))
    assert out.schema.field("r").dtype == DType.list_(DType.int32())
    assert out.to_pydict()["r"] == [[2, None, 0], None, [3]]


def test_lambda_variable_shadows_a_column(cpu_session):
    df = cpu_session.create_dataframe(
        {"a": [[1, 2], [3]], "x": [100, 200]}, dtypes={"a": L_I64, "x": I64})
    cpu_session.register("t", df)
    out = cpu_session.sql(
        "SELECT transform(a, x -> x + 1) AS t, x + 1 AS y, "
        "filter(a, x -> x > 1) AS f FROM t").to_pydict()
    assert out["t"] == [[2, 3], [4]]
    assert out["y"] == [101, 201]
    assert out["f"] == [[2], [3]]
    # in the DSL the variable is an object, so col("x") stays the column
    assert _one(df, col("a").transform(lambda x: x + col("x"))) == \
        [[101, 102], [203]]


def test_sibling_lambdas_do_not_collide(cpu_session):
    df = _base_frame(cpu_session)
    a = col("a")
    out = df.select(a.transform(lambda x: x + 1).alias("p"),
                    a.transform(lambda x: x - 1).alias("m")).to_pydict()
    assert out["p"] == [[2, 3, None, 4], [], None, [None], [5, -3]]
    assert out["m"] == [[0, 1, None, 2], [], None, [None], [3, -5]]
    e1, e2 = a.transform(lambda x: x), a.transform(lambda x: x)
    assert e1.function.args[0].column != e2.function.args[0].column


def test_pruning_keeps_outer_references(cpu_session):
    df = cpu_session.create_dataframe(
        {"a": A, "unused": ["u"] * 5, "k": K},
        dtypes={"a": L_I64, "unused": DType.string(), "k": I64})
    e = col("a").transform(lambda x: x + col("k"))
    assert _expr_refs([e]) == {"a", "k"}
    assert _expr_refs([col("a").filter(lambda x, i: i > col("k"))]) == \
        {"a", "k"}
    assert _one(df, e) == BASE[2][2]


def test_str_children_and_types(cpu_session):
    df = _base_frame(cpu_session)
    a = col("a")
    t = a.transform(lambda x: x + 1)
    body = str(col("x") + 1)
    assert str(t) == f"transform(a, x -> {body})"
    f = a.filter(lambda x, i: x > i)
    assert str(f) == f"filter(a, (x, i) -> {col('x') > col('i')})"
    assert str(a.exists(lambda x: x > 1)).startswith("exists(a, x -> ")
    assert str(a.forall(lambda y: y > 1)).startswith("forall(a, y -> ")
    assert isinstance(t, ArrayTransform) and isinstance(f, ArrayFilter)
    assert isinstance(a.exists(lambda x: x > 1), ArrayExists)
    assert isinstance(a.forall(lambda x: x > 1), ArrayForAll)
    assert t.children[0] is a and isinstance(t.children[1], LambdaFunction)
    assert t.children[1].children == (t.function.body,)
    x = t.function.args[0]
    assert isinstance(x, LambdaVariable) and not isinstance(x, type(a))
    assert t.dtype(df.schema) == L_I64
    assert f.dtype(df.schema) == L_I64
    assert a.exists(lambda x: x > 1).dtype(df.schema) == DType.bool_()
    assert a.forall(lambda x: x > 1).dtype(df.schema) == DType.bool_()


def test_non_boolean_predicate_raises(cpu_session):
    df = _base_frame(cpu_session)
    for name in ("filter", "exists", "forall"):
        e = getattr(col("a"), name)(lambda x: x + 1)
        with pytest.raises(TypeError) as ei:
            e.dtype(df.schema)
        assert name in str(ei.value) and str(I64) in str(ei.value)
    with pytest.raises(TypeError, match="transform"):
        col("k").transform(lambda x: x).dtype(df.schema)


def test_dsl_callable_errors():
    a = col("a")
    for name, bad in (("transform", lambda: 1), ("transform",
                                                  lambda x, i, j: x),
                      ("filter", lambda x, i, j: x), ("filter", lambda *x: 1),
                      ("exists", lambda x, i: x), ("forall", lambda x, i: x)):
        with pytest.raises((TypeError, ValueError), match=name):
            getattr(a, name)(bad)
    for name in ("transform", "filter", "exists", "forall"):
        with pytest.raises((TypeError, ValueError), match=name):
            getattr(a, name)(lambda x: [x])
        with pytest.raises((TypeError, ValueError), match=name):
            getattr(a, name)(lambda x: None)
        with pytest.raises((TypeError, ValueError), match=name):
            getattr(a, name)(3)
    # a literal body is fine
    assert str(a.transform(lambda x: 1)) == "transform(a, x -> 1)"


def test_nested_lambda_over_the_outer_variable_is_refused(cpu_session):
    with pytest.raises(NotImplementedError, match="exists"):
        col("a").transform(
            lambda x: col("b").exists(lambda y: y > x))
    # one that does not refer to the outer variable works
    df = cpu_session.create_dataframe(
        {"a": [[1, 2], []], "b": [[5], [0]]}, dtypes={"a": L_I64, "b": L_I64})
    e = col("a").transform(lambda x: col("b").exists(lambda y: y > 1))
    assert _one(df, e) == [[True, True], []]


def test_parser_errors(cpu_session):
    cpu_session.register("t", _base_frame(cpu_session))
    for q, name in (("transform(a)", "transform"),
                    ("filter(a, x -> x > 1, 3)", "filter"),
                    ("exists()", "exists"),
                    ("forall(a, x -> x > 1, x -> x > 2)", "forall"),
                    ("exists(a, (x, i) -> x > i)", "exists"),
                    ("forall(a, (x, i) -> x > i)", "forall"),
                    ("transform(a, (x, i, j) -> x)", "transform"),
                    ("transform(a, k)", "transform"),
                    ("filter(a, k > 1)", "filter"),
                    ("exists(x -> x > 1, a)", "exists")):
        with pytest.raises(ValueError, match=name):
            cpu_session.sql(f"SELECT {q} AS r FROM t")
    with pytest.raises(ValueError, match="comparator lambdas"):
        cpu_session.sql("SELECT array_sort(a, a) AS r FROM t")
    # '->' is one token, '-' and '>' still are their own
    out = cpu_session.sql(
        "SELECT k - 1 AS m, k > -1 AS g FROM t").to_pydict()
    assert out["m"] == [9, 19, 29, 39, 49] and out["g"] == [True] * 5


def test_tagger(session):
    D = decimal.Decimal
    i64 = session.create_dataframe({"a": A, "k": K},
                                   dtypes={"a": L_I64, "k": I64})
    strs = session.create_dataframe({"a": [["x.y", None]]},
                                    dtypes={"a": L_STR})
    d128 = session.create_dataframe(
        {"a": [[D("1.50"), None]]},
        dtypes={"a": DType.list_(DType.decimal(30, 2))})
    nested = session.create_dataframe({"a": [[[1], None]]},
                                      dtypes={"a": DType.list_(L_I64)})
    t = Tagger(session.conf)
    a = col("a")
    for e in (a.transform(lambda x, i: x + i + col("k")),
              a.filter(lambda x: x > col("k")), a.exists(lambda x: x > 1),
              a.forall(lambda x: x.is_null())):
        assert t.expr_reasons(e, i64.schema) == [], str(e)
    for e in (a.transform(lambda x: x.length()),
              a.filter(lambda x: x.length() > 2),
              a.exists(lambda x: x > "k"), a.forall(lambda x: x.is_null())):
        assert t.expr_reasons(e, strs.schema) == [], str(e)
    for e in (a.transform(lambda x: x), a.filter(lambda x: x.is_null()),
              a.exists(lambda x: x.is_null()),
              a.forall(lambda x: x.is_null())):
        assert t.expr_reasons(e, d128.schema) == [], str(e)
    for name in ("transform", "filter", "exists", "forall"):
        if name == "transform":
            e = a.transform(lambda x: substring_index(x, ".", 1))
        else:
            e = getattr(a, name)(
                lambda x: substring_index(x, ".", 1) == "x")
        reasons = t.expr_reasons(e, strs.schema)
        assert len(reasons) == 1 and reasons[0].startswith(name), reasons
        reasons = t.expr_reasons(
            getattr(a, name)(lambda x: x.is_null()), nested.schema)
        assert len(reasons) == 1 and name in reasons[0] \
            and "nested" in reasons[0], reasons
    # a nested result type, and a disabled expression
    reasons = t.expr_reasons(a.transform(lambda x: col("a")), i64.schema)
    assert any("nested" in r and "transform" in r for r in reasons), reasons
    conf = session.conf.copy()
    conf.set("spark.rapids.sql.expression.ArrayFilter", False)
    reasons = Tagger(conf).expr_reasons(a.filter(lambda x: x > 1), i64.schema)
    assert reasons == ["expression ArrayFilter disabled by conf"]


def test_docgen_lists_lambda_functions(tmp_path, monkeypatch):
    from spark_rapids_amd.tools import docgen

    monkeypatch.setattr(docgen, "REPO", str(tmp_path))
    docgen.main()
    text = open(os.path.join(str(tmp_path), "docs",
                             "supported_ops.md")).read()
    rows = {ln.split("|")[1].strip(): ln.split("|")[3].strip()
            for ln in text.splitlines() if ln.startswith("| ")}
    for name in ("ArrayTransform", "ArrayFilter", "ArrayExists",
                 "ArrayForAll"):
        assert rows.get(name) == "GPU*", (name, rows.get(name))


# ---------------------------------------------------------------------------
# GPU vs CPU
# ---------------------------------------------------------------------------

def _int_rows(lengths, rng, null_rows=0.0, lo=-3, hi=3):
    rows = []
    for ln in lengths:
        if rng.random() < null_rows:
            rows.append(None)
        else:
            rows.append([None if rng.random() < 0.1 else
                         int(rng.integers(lo, hi + 1)) for _ in range(ln)])
    return rows


def _flat_pred(rows, fn):
    """Host BOOL column with fn(x) for every element (None stays None)."""
    return Column.from_pylist([None if x is None else fn(x)
                               for v in rows if v is not None for x in v],
                              DType.bool_())


def _same_rows(dev, host):
    rg, pg = ops.list_element_rows(dev)
    rh, ph = ops.list_element_rows(host)
    assert rg.is_cuda and pg.is_cuda
    assert rg.cpu().to_pylist() == rh.to_pylist()
    assert pg.cpu().to_pylist() == ph.to_pylist()
    only, none = ops.list_element_rows(dev, with_pos=False)
    assert none is None and only.cpu().to_pylist() == rh.to_pylist()


@pytest.mark.gpu
def test_gpu_row_search_and_positions():
    rng = np.random.default_rng(7)
    lengths = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 300] * 3
    rng.shuffle(lengths)
    rows = _int_rows(lengths, rng, null_rows=0.15)
    rows[4] = None
    assert any(v is None for v in rows) and any(v == [] for v in rows)
    _same_rows(Column.from_pylist(rows, L_I64).cuda(),
               Column.from_pylist(rows, L_I64))
    for rows in ([[5, None, 7]], [[], None, [], [1, 2, 3, 4]], [[9]]):
        _same_rows(Column.from_pylist(rows, L_I64).cuda(),
                   Column.from_pylist(rows, L_I64))


@pytest.fixture(scope="module")
def wide_rows():
    """About 70,000 rows of 0..16 elements: past the 2048 * 256 threads of a
    capped flat grid, so the element kernels take their grid stride."""
    rng = np.random.default_rng(70)
    n = 70_000
    lens = rng.integers(0, 17, n)
    vals = rng.integers(-50, 51, int(lens.sum()))
    nulls = rng.random(len(vals)) < 0.1
    flat = [None if z else int(v) for v, z in zip(vals, nulls)]
    rows, p = [], 0
    for r, ln in enumerate(lens):
        rows.append(None if r % 97 == 5 else flat[p:p + ln])
        p += ln
    assert sum(len(v) for v in rows if v) > 2048 * 256
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("text", ["transform(a, (x, i) -> x * 2 + i)",
                                  "filter(a, x -> x % 3 = 0)"])
def test_gpu_grid_stride(text, wide_rows, gpu_session, cpu_session):
    out = []
    for s in (gpu_session, cpu_session):
        s.register("t", s.create_dataframe({"a": wide_rows},
                                           dtypes={"a": L_I64}))
        out.append(s.sql(f"SELECT {text} AS r FROM t").to_pydict()["r"])
    assert out[0] == out[1]


def _tri_rows(n, max_len, rng):
    """Rows for x > 0 over values from -3..3 in which every outcome of
    exists and forall occurs at every length: a row draws from the positive
    values, from the others or from all of them, with or without nulls."""
    rows = []
    for r in range(n):
        if n > 3 and r in (1, 2):  # always an empty and a null row
            rows.append([] if r == 1 else None)
            continue
        if r != n // 2 and rng.random() < 0.1:
            rows.append(None)
            continue
        ln = max_len if r == n // 2 else int(rng.integers(0, max_len + 1))
        lo, hi = [(1, 3), (-3, 0), (-3, 3), (-3, 3)][int(rng.integers(0, 4))]
        p_null = [0.0, 0.1][int(rng.integers(0, 2))]
        rows.append([None if rng.random() < p_null else
                     int(rng.integers(lo, hi + 1)) for _ in range(ln)])
    return rows


def _check_bool_reduce(rows, need_all):
    host = Column.from_pylist(rows, L_I64)
    pred = _flat_pred(rows, lambda x: x > 0)
    dev, dpred = host.cuda(), pred.cuda()
    for fn in (ops.array_exists, ops.array_forall):
        want = fn(host, pred).to_pylist()
        if need_all:
            assert {True, False, None} <= set(want), fn.__name__
        got = fn(dev, dpred)
        assert got.cpu().to_pylist() == want, fn.__name__
        assert got.null_count == want.count(None)


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [5, 8, 9, 16, 29, 32, 33, 64, 200])
def test_gpu_exists_forall_validity_words(max_len):
    """203 rows are three full validity words and a partial one; the lane
    group (8/16/32/64) follows the mean length and strides over the rows
    that are longer, up to max_len exactly."""
    rows = _tri_rows(203, max_len, np.random.default_rng(max_len))
    assert max(len(v) for v in rows if v is not None) == max_len
    assert None in rows and [] in rows
    _check_bool_reduce(rows, need_all=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_gpu_exists_forall_row_counts(n):
    _check_bool_reduce(_tri_rows(n, 6, np.random.default_rng(n)),
                       need_all=n > 1)


def _view(big, dt, lo, m):
    # word-aligned start keeps the validity view aligned
    return Column(dt, m, big.data,
                  None if big.validity is None else big.validity[lo // 8:],
                  big.offsets[lo:lo + m + 1], None, big.child)


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
                vals.append([NAN, -0.0, 0.0, 1.5, -2.5, float("inf"), 7.25,
                             -1.0][int(rng.integers(0, 8))])
            else:
                vals.append(int(rng.integers(-6, 7)))
        rows.append(vals)
    return rows


def _four_for(kind):
    a, k = col("a"), col("k")
    if kind == "string":
        return [a.transform(lambda x, i: x.length() + i + k),
                a.filter(lambda x, i: x.length() > i),
                a.exists(lambda x: x.length() > 2),
                a.forall(lambda x: x.length() < 12)]
    if kind == "double":
        return [a.transform(lambda x, i: x * 2.0 + i + k),
                a.filter(lambda x, i: x > i),
                a.exists(lambda x: x > 1.5), a.forall(lambda x: x > -2.0)]
    return [a.transform(lambda x, i: x * 2 + i + k),
            a.filter(lambda x, i: x > i), a.exists(lambda x: x > 4),
            a.forall(lambda x: x > -5)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,kind", [(L_I64, "int64"), (L_STR, "string")])
def test_gpu_nonzero_first_offset(dt, kind):
    """A zero-copy row range of a larger LIST column: offsets start past 0
    and the child holds elements of rows outside the range. The transform
    uses the position and an outer column, so rowid and pos must both be
    rebased."""
    rows = _short_lists(kind, 400, 31)
    lo, m = 64, 200
    big = Column.from_pylist(rows, dt).cuda()
    view = _view(big, dt, lo, m)
    assert int(view.offsets[0].item()) > 0
    keys = Column.from_pylist(list(range(1000, 1000 + m)), I64)
    schema = Schema([Field("a", dt), Field("k", I64)])
    dev = ColumnBatch([view, keys.cuda()], m)
    host = ColumnBatch([Column.from_pylist(rows[lo:lo + m], dt), keys], m)
    before = (big.offsets.clone(), big.child.data.clone())
    _same_rows(view, host.columns[0])
    for e in _four_for(kind):
        got = e.eval(dev, schema).cpu().to_pylist()
        want = e.eval(host, schema).to_pylist()
        assert repr(got) == repr(want), str(e)
    # inputs are never modified
    assert bool((before[0] == big.offsets).all())
    assert bool((before[1] == big.child.data).all())


def _both(gpu_session, cpu_session, data, dtypes, texts):
    out = []
    for s in (gpu_session, cpu_session):
        s.register("t", s.create_dataframe(data, dtypes=dtypes))
        sel = ", ".join(f"{q} AS c{j}" for j, q in enumerate(texts))
        out.append(s.sql(f"SELECT {sel} FROM t").to_pydict())
    return out


@pytest.mark.gpu
def test_gpu_double_nan_negative_zero_and_null(gpu_session, cpu_session):
    a = [[0.0, 1.0, -1.0, None, NAN], [], None, [-0.0, 2.0], [3.0, None]]
    y = [0.0, 1.0, 2.0, -1.0, None]
    got, want = _both(
        gpu_session, cpu_session, {"a": a, "y": y},
        {"a": L_F64, "y": DType.float64()},
        ["transform(a, x -> x / y)", "transform(a, x -> x * y)",
         "filter(a, x -> x / y > 0)", "exists(a, x -> x * y < 0)",
         "forall(a, x -> x * y <= 0)"])
    assert repr(got) == repr(want)
    flat = [x for v in want["c1"] if v for x in v]
    assert any(x is None for x in flat)
    assert any(x is not None and x != x for x in flat)
    assert any(x == 0 and repr(x) == "-0.0" for x in flat if x is not None)


@pytest.mark.gpu
def test_gpu_string_elements(gpu_session, cpu_session):
    a = _short_lists("string", 300, 5) + [["commonprefix", None], [], None]
    got, want = _both(
        gpu_session, cpu_session, {"a": a}, {"a": L_STR},
        ["filter(a, x -> length(x) > 2)", "transform(a, x -> concat(x, 'z'))",
         "exists(a, x -> x LIKE 'common%')", "transform(a, x -> length(x))"])
    assert got == want
    assert {True, False, None} <= set(want["c2"])


@pytest.mark.gpu
def test_gpu_int32_date_decimal64_against_an_outer_column(gpu_session,
                                                          cpu_session):
    rng = np.random.default_rng(9)
    D = decimal.Decimal
    pools = {
        "int32": (DType.int32(), [-2 ** 31, 2 ** 31 - 1, 0, -1, 5, 6]),
        "date": (DType.date32(), [-1, 0, 10957, 19000, 5]),
        "decimal64": (DType.decimal(12, 2),
                      [D("-99.50"), D("0.00"), D("12345.67"), D("0.01")]),
    }
    for kind, (et, pool) in pools.items():
        def pick():
            return pool[int(rng.integers(0, len(pool)))]
        a = [None] + [[None if rng.random() < 0.1 else pick()
                       for _ in range(ln)] for ln in (0, 1, 3, 9, 70)]
        k = [pick() for _ in a]
        k[2] = None
        got, want = _both(
            gpu_session, cpu_session, {"a": a, "k": k},
            {"a": DType.list_(et), "k": et},
            ["filter(a, x -> x > k)", "exists(a, x -> x >= k)",
             "forall(a, x -> x <= k)", "transform(a, x -> x = k)"])
        assert repr(got) == repr(want), kind


@pytest.mark.gpu
def test_gpu_decimal128_elements(gpu_session, cpu_session):
    D = decimal.Decimal
    dt = DType.decimal(30, 2)
    a = [[D("2.50"), None, D("-1.25")], None, [], [D("1.00")]]
    bound = lit(D("1.00"), dt)
    exprs = [col("a").filter(lambda x: x > bound).alias("f"),
             col("a").exists(lambda x: x > bound).alias("e"),
             col("a").forall(lambda x: x > bound).alias("g"),
             col("a").transform(lambda x: x.is_null()).alias("t")]
    out = []
    for s in (gpu_session, cpu_session):
        df = s.create_dataframe({"a": a}, dtypes={"a": DType.list_(dt)})
        out.append(df.select(*exprs).to_pydict())
    assert repr(out[0]) == repr(out[1])
    assert out[1]["f"] == [[D("2.50")], None, [], []]
    assert out[1]["e"] == [True, None, False, False]


@pytest.mark.gpu
def test_gpu_predicate_validity_forms():
    rows = _int_rows([3, 0, 5, 1, 70, 2], np.random.default_rng(2))
    rows[3] = None
    host = Column.from_pylist(rows, L_I64)
    total = sum(len(v) for v in rows if v)
    plain = Column.from_pylist([j % 3 == 0 for j in range(total)],
                               DType.bool_())
    assert plain.validity is None
    nulls = Column.from_pylist([None] * total, DType.bool_())
    for pred in (plain, nulls):
        for fn in (ops.array_filter, ops.array_exists, ops.array_forall):
            got = fn(host.cuda(), pred.cuda()).cpu().to_pylist()
            assert got == fn(host, pred).to_pylist(), fn.__name__
    assert ops.array_exists(host, nulls).to_pylist() == \
        [None, False, None, None, None, None]


@pytest.mark.gpu
def test_gpu_empty_inputs(gpu_session, cpu_session):
    for rows in ([], [[], None, []], [None]):
        dev = Column.from_pylist(rows, L_I64).cuda()
        host = Column.from_pylist(rows, L_I64)
        schema = Schema([Field("a", L_I64)])
        for e in (col("a").transform(lambda x, i: x + i),
                  col("a").transform(lambda x: x > 1),
                  col("a").filter(lambda x: x > 1),
                  col("a").exists(lambda x: x > 1),
                  col("a").forall(lambda x: x > 1)):
            got = e.eval(ColumnBatch([dev], len(rows)), schema)
            want = e.eval(ColumnBatch([host], len(rows)), schema)
            assert got.is_cuda and got.dtype == want.dtype == e.dtype(schema)
            assert got.cpu().to_pylist() == want.to_pylist(), (str(e), rows)
        rowid, pos = ops.list_element_rows(dev)
        assert rowid.size == 0 and pos.size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("dt,kind", [(L_I64, "int64"), (L_F64, "double"),
                                     (L_STR, "string")])
def test_gpu_random_sweep(dt, kind, seed, gpu_session, cpu_session):
    rows = _short_lists(kind, 3000, seed)
    k = [int(v) for v in np.random.default_rng(seed).integers(-3, 4, 3000)]
    exprs = [e.alias(f"c{j}") for j, e in enumerate(_four_for(kind))]
    out = []
    for s in (gpu_session, cpu_session):
        df = s.create_dataframe({"a": rows, "k": k},
                                dtypes={"a": dt, "k": I64})
        out.append(df.select(*exprs).to_pydict())
    for name in out[1]:
        assert repr(out[0][name]) == repr(out[1][name]), (kind, name)


@pytest.mark.gpu
def test_gpu_plan_placement(gpu_session, cpu_session):
    data = {"a": [["x.y", None, "abc"], None, []], "k": [1, 2, 3]}
    dtypes = {"a": L_STR, "k": I64}
    clean = [col("a").transform(lambda x, i: x.length() + i + col("k")),
             col("a").filter(lambda x: x.length() > 2),
             col("a").exists(lambda x: x.length() > 2),
             col("a").forall(lambda x: x.length() > 2)]
    unclean = col("a").transform(lambda x: substring_index(x, ".", 1))
    df = gpu_session.create_dataframe(data, dtypes=dtypes)
    tree = df.select(*clean).physical_plan().tree_string()
    assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
    text = df.select(unclean).explain()
    assert "CpuProject[transform(" in text, text
    assert "GpuProject[transform(" not in text, text
    assert "transform lambda body: " in text, text
    cdf = cpu_session.create_dataframe(data, dtypes=dtypes)
    for e in clean + [unclean]:
        assert _one(df, e) == _one(cdf, e), str(e)
    assert _one(cdf, unclean) == [["x", None, "abc"], None, []]
