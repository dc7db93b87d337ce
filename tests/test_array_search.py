"""array_position / array_remove / slice / array_repeat (reference analogue:
GpuArrayPosition, GpuArrayRemove, GpuSlice, GpuArrayRepeat in
collectionOperations.scala).

Element equality is array_distinct's (NaN equals NaN, -0.0 equals 0.0, strings
by their UTF-8 bytes), except that a null element equals no needle. The CPU
implementations are the oracle and are pinned by the hand-written expectations
below; the GPU tests compare a GPU session, or the GPU backend directly, with
them through repr() of whole results, so that NaN and the sign of a zero count.
"""
import decimal
import math
import os

import numpy as np
import pytest
import torch

import spark_rapids_amd as sr
from spark_rapids_amd import (Column, DType, array_position, array_remove,
                              array_repeat, col, lit, slice_)
from spark_rapids_amd import ops
from spark_rapids_amd.column import make_validity
from spark_rapids_amd.plan.overrides import Tagger

NAN = float("nan")
INF = float("inf")
I32, I64, F64, STR = (DType.int32(), DType.int64(), DType.float64(),
                      DType.string())
L_I32, L_I64, L_F64, L_STR = (DType.list_(t) for t in (I32, I64, F64, STR))
IMAX = 2 ** 31 - 1
START_MSG = ("Unexpected value for start in function slice: "
             "SQL array indices start at 1.")
LENGTH_MSG = ("Unexpected value for length in function slice: "
              "length must be greater than or equal to 0.")


def _frame(session, data, dtypes):
    return session.create_dataframe(data, dtypes=dtypes)


def _select(session, data, dtypes, **exprs):
    df = _frame(session, data, dtypes)
    return df.select(*[e.alias(k) for k, e in exprs.items()]).to_pydict()


# ---------------------------------------------------------------------------
# CPU: hand-written expectations
# ---------------------------------------------------------------------------

A = [[1, 2, None, 2], None, [], [None, None], [3], [2]]
V = [2, 1, 1, 1, None, 2]


def test_position_and_remove_null_rules(cpu_session):
    out = _select(cpu_session, {"a": A, "v": V}, {"a": L_I64, "v": I64},
                  p=col("a").array_position(col("v")),
                  r=col("a").array_remove(col("v")))
    # null array, empty array, only null elements, null needle
    assert out["p"] == [2, None, 0, 0, None, 1]
    assert out["r"] == [[1, None], None, [], [None, None], None, []]


def test_position_and_remove_floats(cpu_session):
    data = {"a": [[1.0, NAN, -0.0, NAN], [1.0, -0.0], [-0.0, 1.0, 0.0],
                  [-0.0, 1.0, NAN]],
            "v": [NAN, 0.0, 0.0, 1.0]}
    out = _select(cpu_session, data, {"a": L_F64, "v": F64},
                  p=col("a").array_position(col("v")),
                  r=col("a").array_remove(col("v")))
    assert out["p"] == [2, 2, 1, 2]
    assert repr(out["r"]) == repr([[1.0, -0.0], [1.0], [1.0], [-0.0, NAN]])
    # a zero that survives another needle keeps its sign
    assert math.copysign(1.0, out["r"][3][0]) == -1.0
    assert math.copysign(1.0, out["r"][0][1]) == -1.0


def test_position_and_remove_strings(cpu_session):
    data = {"a": [["commonprefix1", "commonprefix", "commonprefix1"],
                  ["a", "", None, ""],
                  ["e", "é", "éé"],
                  ["", "x"]],
            "v": ["commonprefix", "", "é", "commonprefi"]}
    out = _select(cpu_session, data, {"a": L_STR, "v": STR},
                  p=col("a").array_position(col("v")),
                  r=col("a").array_remove(col("v")))
    assert out["p"] == [2, 2, 2, 0]
    assert out["r"] == [["commonprefix1", "commonprefix1"], ["a", None],
                        ["e", "éé"], ["", "x"]]
    one = _select(cpu_session, {"a": [["commonprefix", "commonprefix1"]]},
                  {"a": L_STR},
                  p=col("a").array_position("commonprefix1"),
                  r=col("a").array_remove("commonprefix1"))
    assert one == {"p": [2], "r": [["commonprefix"]]}


FIVE = [1, 2, 3, 4, 5]
SLICES = [((2, 2), [2, 3]), ((-2, 5), [4, 5]), ((6, 1), []), ((-6, 2), []),
          ((5, 0), []), ((1, 100), FIVE), ((IMAX, IMAX), []),
          ((-5, 1), [1]), ((5, 1), [5]), ((-(2 ** 31), IMAX), [])]


def test_slice_cases(cpu_session):
    exprs = {f"s{i}": col("a").slice(s, ln)
             for i, ((s, ln), _) in enumerate(SLICES)}
    out = _select(cpu_session, {"a": [FIVE]}, {"a": L_I64}, **exprs)
    for i, (args, want) in enumerate(SLICES):
        assert out[f"s{i}"] == [want], args


def test_slice_null_rules(cpu_session):
    data = {"a": [FIVE, None, FIVE, FIVE, [], [None, 7]],
            "s": [2, 1, None, 1, 1, -1],
            "n": [2, 1, 1, None, 3, 4]}
    out = _select(cpu_session, data, {"a": L_I64, "s": I32, "n": I32},
                  x=col("a").slice(col("s"), col("n")))
    assert out["x"] == [[2, 3], None, None, None, [], [7]]


def _slice_rows(session, a, s, n):
    return _select(session, {"a": a, "s": s, "n": n},
                   {"a": L_I64, "s": I32, "n": I32},
                   x=col("a").slice(col("s"), col("n")))["x"]


def _check_slice_errors(session):
    with pytest.raises(ValueError) as ei:
        _slice_rows(session, [FIVE, FIVE], [1, 0], [1, 1])
    assert str(ei.value) == START_MSG
    with pytest.raises(ValueError) as ei:
        _slice_rows(session, [FIVE, FIVE], [1, 2], [-1, 1])
    assert str(ei.value) == LENGTH_MSG
    # start is checked before length, also across rows
    with pytest.raises(ValueError) as ei:
        _slice_rows(session, [FIVE, FIVE], [1, 0], [-1, 1])
    assert str(ei.value) == START_MSG
    with pytest.raises(ValueError) as ei:
        _select(session, {"a": [FIVE]}, {"a": L_I64}, x=col("a").slice(0, 1))
    assert str(ei.value) == START_MSG
    with pytest.raises(ValueError) as ei:
        _select(session, {"a": [FIVE]}, {"a": L_I64}, x=col("a").slice(1, -1))
    assert str(ei.value) == LENGTH_MSG


def _check_slice_errors_masked(session):
    """A zero start or a negative length in a row where another operand is
    null is never looked at."""
    got = _slice_rows(session, [None, FIVE, FIVE, None, FIVE],
                      [0, 0, None, 1, 2], [1, None, -1, -5, 1])
    assert got == [None, None, None, None, [2]]


def test_slice_errors(cpu_session):
    _check_slice_errors(cpu_session)


def test_slice_errors_masked_by_null(cpu_session):
    _check_slice_errors_masked(cpu_session)


def test_array_repeat_rules(cpu_session):
    data = {"e": [7, 8, None, 9, 10], "s": ["ab", "", None, "é", "x"],
            "c": [3, 0, 2, None, -1]}
    out = _select(cpu_session, data, {"e": I64, "s": STR, "c": I32},
                  e=array_repeat(col("e"), col("c")),
                  s=array_repeat(col("s"), col("c")))
    # a null element repeats as nulls and the row is not null
    assert out["e"] == [[7, 7, 7], [], [None, None], None, []]
    assert out["s"] == [["ab", "ab", "ab"], [], [None, None], None, []]


def test_array_repeat_overflow(cpu_session):
    with pytest.raises(OverflowError):
        _select(cpu_session, {"e": [1, 2], "c": [IMAX, 1]},
                {"e": I64, "c": I32}, x=array_repeat(col("e"), col("c")))


def test_operand_forms(cpu_session):
    """Needle, start, length and count as a column, a literal, a computed
    expression and a python scalar."""
    data = {"a": [[1, 2, 3, 2], [2]], "v": [2, 2], "k": [2, 2]}
    dts = {"a": L_I64, "v": I64, "k": I32}
    a = col("a")
    out = _select(
        cpu_session, data, dts,
        p_col=a.array_position(col("v")),
        p_lit=a.array_position(lit(2, I64)),
        p_null=a.array_position(lit(None)),    # an untyped null literal
        p_py=a.array_position(2),
        p_expr=a.array_position(col("v") + lit(1, I64)),
        r_col=a.array_remove(col("v")), r_py=a.array_remove(2),
        r_fn=array_remove(a, lit(2, I64)), p_fn=array_position(a, 3),
        s_col=a.slice(col("k"), col("k")), s_py=a.slice(2, 2),
        s_lit=a.slice(lit(2), lit(2)), s_fn=slice_(a, col("k"), 2),
        s_i64=a.slice(col("v"), col("v")),     # cast to INT32
        s_expr=a.slice(col("k") - 1, col("k") + 1),
        t_col=array_repeat(col("v"), col("k")), t_py=array_repeat(col("v"), 2),
        t_lit=array_repeat(lit("z"), lit(2)), t_i64=array_repeat(5, col("v")))
    for k in ("p_col", "p_lit", "p_py"):
        assert out[k] == [2, 1], k
    assert out["p_null"] == [None, None]
    assert out["p_expr"] == [3, 0] and out["p_fn"] == [3, 0]
    for k in ("r_col", "r_py", "r_fn"):
        assert out[k] == [[1, 3], []], k
    for k in ("s_col", "s_py", "s_lit", "s_fn", "s_i64"):
        assert out[k] == [[2, 3], []], k
    assert out["s_expr"] == [[1, 2, 3], [2]]
    assert out["t_col"] == out["t_py"] == [[2, 2], [2, 2]]
    assert out["t_lit"] == [["z", "z"]] * 2 and out["t_i64"] == [[5, 5]] * 2
    # an int scalar is coerced to a floating element type
    f = _select(cpu_session, {"a": [[1.0, 2.0]]}, {"a": L_F64},
                p=col("a").array_position(2), r=col("a").array_remove(1))
    assert f == {"p": [2], "r": [[2.0]]}
    # a null literal of any type is a null needle
    n = _select(cpu_session, {"a": [[1]]}, {"a": L_I64},
                p=col("a").array_position(None))
    assert n == {"p": [None]}


D = decimal.Decimal
DEC_ROWS = [[D("5.00"), D("0.05"), None, D("5.00")], [D("0.05")], [D("-5.00")]]


def _check_decimal_scalar_needles(session, et):
    """A python scalar against decimal elements stands for its value: 5 is
    5.00, never the unscaled 0.05."""
    dt = DType.list_(et)
    a = col("a")
    out = _select(session, {"a": DEC_ROWS, "v": [D("5.00")] * 3},
                  {"a": dt, "v": et},
                  p_int=a.array_position(5), p_dec=a.array_position(D("5")),
                  p_dec2=a.array_position(D("5.00")),
                  p_float=a.array_position(5.0), p_col=a.array_position(col("v")),
                  p_small=a.array_position(D("0.05")),
                  p_fsmall=a.array_position(0.05),
                  p_neg=a.array_position(-5),
                  r_int=a.array_remove(5), r_dec=a.array_remove(D("5.00")),
                  r_small=a.array_remove(D("0.05")))
    for k in ("p_int", "p_dec", "p_dec2", "p_float", "p_col"):
        assert out[k] == [1, 0, 0], k
    assert out["p_small"] == out["p_fsmall"] == [2, 1, 0]
    assert out["p_neg"] == [0, 0, 1]
    assert out["r_int"] == out["r_dec"] == [[D("0.05"), None], [D("0.05")],
                                           [D("-5.00")]]
    assert out["r_small"] == [[D("5.00"), None, D("5.00")], [], [D("-5.00")]]


@pytest.mark.parametrize("et", [DType.decimal(12, 2), DType.decimal(30, 2)],
                         ids=["decimal64", "decimal128"])
def test_decimal_scalar_needles(et, cpu_session):
    _check_decimal_scalar_needles(cpu_session, et)
    df = _frame(cpu_session, {"a": DEC_ROWS}, {"a": DType.list_(et)})
    # values the element type cannot hold exactly are refused, not rounded
    for bad in (D("5.001"), 0.125, 10 ** et.precision, "5", float("nan")):
        with pytest.raises(TypeError):
            col("a").array_position(bad).dtype(df.schema)
    cpu_session.register("d", df)
    got = cpu_session.sql("SELECT array_position(a, 5) AS p, "
                          "array_position(a, 5.00) AS q, "
                          "array_remove(a, 0.05) AS r FROM d").to_pydict()
    assert got["p"] == got["q"] == [1, 0, 0]
    assert got["r"] == [[D("5.00"), None, D("5.00")], [], [D("-5.00")]]


def test_type_errors(cpu_session):
    df = _frame(cpu_session, {"a": [[1]], "v32": [1], "s": ["x"], "f": [1.0],
                              "i": [1]},
                {"a": L_I64, "v32": I32, "s": STR, "f": F64, "i": I64})
    a = col("a")
    for e in (a.array_position(col("s")), a.array_remove(col("f")),
              a.array_position(col("v32")),    # no implicit widening,
              a.array_position(lit(1)),        # of a typed literal either
              a.array_remove(lit(1.0)),
              a.array_position("x"), a.array_remove(1.5),
              col("i").array_position(1),      # not an array
              a.slice(col("f"), 1), a.slice(1, col("s")),
              col("i").slice(1, 1), array_repeat(a, col("f"))):
        with pytest.raises(TypeError):
            e.dtype(df.schema)
    with pytest.raises(TypeError) as ei:
        a.array_position(col("s")).dtype(df.schema)
    assert str(L_I64) in str(ei.value) and str(STR) in str(ei.value)
    with pytest.raises(TypeError):
        df.select(a.array_remove(col("s")).alias("x")).to_pydict()
    for bad in (lambda: a.slice(1.5, 1), lambda: a.slice(1, "2"),
                lambda: array_repeat(a, 2.0), lambda: a.slice(True, 1)):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(ValueError):
        a.slice(2 ** 31, 1)


def test_expression_types_and_names(cpu_session):
    df = _frame(cpu_session, {"a": [["x"]], "v": ["x"], "k": [1]},
                {"a": L_STR, "v": STR, "k": I32})
    a, v, k = col("a"), col("v"), col("k")
    assert a.array_position(v).dtype(df.schema) == I64
    assert a.array_remove(v).dtype(df.schema) == L_STR
    assert a.slice(k, 2).dtype(df.schema) == L_STR
    assert array_repeat(v, k).dtype(df.schema) == L_STR
    assert array_repeat(a, k).dtype(df.schema) == DType.list_(L_STR)
    assert str(a.array_position(v)) == "array_position(a, v)"
    assert str(a.array_remove("q")) == "array_remove(a, 'q')"
    assert str(a.slice(k, 2)) == "slice(a, k, 2)"
    assert str(array_repeat(v, k)) == "array_repeat(v, k)"
    assert a.array_position(v).children == (a, v)
    assert a.slice(k, k).children == (a, k, k)
    assert array_repeat(v, k).children == (v, k)
    assert sr.slice_ is slice_ and sr.array_repeat is array_repeat


def test_sql_functions(cpu_session):
    data = {"a": A, "v": V, "s": [1, 2, -1, 1, -3, 1],
            "n": [2, 1, 0, None, 1, 5]}
    dts = {"a": L_I64, "v": I64, "s": I32, "n": I32}
    df = _frame(cpu_session, data, dts)
    cpu_session.register("t", df)
    got = cpu_session.sql(
        "SELECT array_position(a, v) AS p, array_position(a, 2) AS p2, "
        "array_remove(a, v) AS r, array_remove(a, 2) AS r2, "
        "slice(a, s, n) AS s1, slice(a, -2, 5) AS s2, slice(a, 2, 1) AS s3, "
        "array_repeat(v, n) AS t, array_repeat('ab', 2) AS t2, "
        "array_repeat(v, -1) AS t3 FROM t").to_pydict()
    a = col("a")
    want = _select(cpu_session, data, dts,
                   p=a.array_position(col("v")), p2=a.array_position(2),
                   r=a.array_remove(col("v")), r2=a.array_remove(2),
                   s1=a.slice(col("s"), col("n")), s2=a.slice(-2, 5),
                   s3=a.slice(2, 1), t=array_repeat(col("v"), col("n")),
                   t2=array_repeat(lit("ab"), 2),
                   t3=array_repeat(col("v"), -1))
    assert got == want
    assert got["s2"][0] == [None, 2] and got["t3"][0] == []


def test_sql_argument_count(cpu_session):
    cpu_session.register("t", _frame(cpu_session, {"a": A, "v": V},
                                     {"a": L_I64, "v": I64}))
    for q in ("array_position(a)", "array_remove(a, v, v)",
              "array_repeat(v)"):
        with pytest.raises(ValueError, match="two arguments"):
            cpu_session.sql(f"SELECT {q} AS x FROM t")
    for q in ("slice(a, 1)", "slice(a, 1, 2, 3)"):
        with pytest.raises(ValueError, match="three arguments"):
            cpu_session.sql(f"SELECT {q} AS x FROM t")


def _four(a, v, k):
    return [a.array_position(v), a.array_remove(v), a.slice(k, k),
            array_repeat(v, k)]


def test_tagger_element_types(session):
    def frame(rows, et):
        return _frame(session, {"a": [rows], "v": [rows[0]], "k": [1]},
                      {"a": DType.list_(et), "v": et, "k": I32})

    t = Tagger(session.conf)
    a, v, k = col("a"), col("v"), col("k")
    for rows, et in (([1, None], I64), ([1.5, NAN], F64), (["x", ""], STR)):
        df = frame(rows, et)
        for e in _four(a, v, k):
            assert t.expr_reasons(e, df.schema) == [], (str(e), et)
    d128 = frame([decimal.Decimal("1.5"), None], DType.decimal(30, 2))
    nested = frame([[1], None], L_I64)
    for e in _four(a, v, k)[:2]:
        for df, word in ((d128, "decimal128"), (nested, "nested")):
            reasons = t.expr_reasons(e, df.schema)
            assert len(reasons) == 1 and word in reasons[0] \
                and "on CPU" in reasons[0], reasons
    # slice and array_repeat never compare elements
    for e in _four(a, v, k)[2:]:
        assert t.expr_reasons(e, d128.schema) == [], str(e)
        reasons = t.expr_reasons(e, nested.schema)
        assert len(reasons) == 1 and "nested" in reasons[0], reasons
    conf = session.conf.copy()
    for name, e in zip(("ArrayPosition", "ArrayRemove", "ArraySlice",
                        "ArrayRepeat"), _four(a, v, k)):
        conf.set(f"spark.rapids.sql.expression.{name}", False)
        reasons = Tagger(conf).expr_reasons(e, frame([1], I64).schema)
        assert reasons == [f"expression {name} disabled by conf"], reasons


def test_docgen_lists_the_functions(tmp_path, monkeypatch):
    from spark_rapids_amd.tools import docgen

    monkeypatch.setattr(docgen, "REPO", str(tmp_path))
    docgen.main()
    text = open(os.path.join(str(tmp_path), "docs",
                             "supported_ops.md")).read()
    rows = {ln.split("|")[1].strip(): ln.split("|")[3].strip()
            for ln in text.splitlines() if ln.startswith("| ")}
    for name in ("ArrayPosition", "ArrayRemove", "Slice", "ArrayRepeat"):
        assert rows.get(name) == "GPU", (name, rows.get(name))


# ---------------------------------------------------------------------------
# GPU vs CPU
# ---------------------------------------------------------------------------

_WORDS = ["", "a", "ab", "abc", "b", "commonprefix", "commonprefix1",
          "commonprefix2", "é", "zz", "commonprefi"]
# (element type, values that meet often, values held back for misses)
_KINDS = {
    "int32": (I32, [-2 ** 31, IMAX, 0, -1, 5, 6, 7], [11, -12]),
    "int64": (I64, [-2 ** 63, 2 ** 63 - 1, 0, -1, 5, 6, 7], [11, -12]),
    "double": (F64, [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.5, 1.7e308],
               [7.25, -1.7e308]),
    "string": (STR, _WORDS[:-2], _WORDS[-2:]),
}


def _elems(kind, rng, ln):
    pool = _KINDS[kind][1]
    return [None if rng.random() < 0.1 else
            pool[int(rng.integers(0, len(pool)))] for _ in range(ln)]


def _search_rows(kind, n, max_len, seed):
    """n rows of 0..max_len elements and a needle per row: a tenth null,
    else half taken from the row (so it matches, usually more than once)
    and half from the values no row holds. When n allows, row 1 reaches
    max_len with its only match in the last place, beyond every lane group
    width, row 2 has its matches in the second half only, and row 3 is a
    null row."""
    rng = np.random.default_rng(seed)
    _, pool, misses = _KINDS[kind]
    a, v = [], []
    for r in range(n):
        row = _elems(kind, rng, int(rng.integers(0, max_len + 1)))
        x = rng.random()
        live = [e for e in row if e is not None]
        if x < 0.1:
            needle = None
        elif x < 0.55 and live:
            needle = live[int(rng.integers(0, len(live)))]
        else:
            needle = misses[int(rng.integers(0, len(misses)))]
        a.append(row)
        v.append(needle)
    if n > 3:
        a[1], v[1] = [pool[-1]] * (max_len - 1) + [pool[-2]], pool[-2]
        half = max_len // 2
        a[2] = [pool[-1]] * half + [pool[-2], None, pool[-2]][:max_len - half]
        v[2] = pool[-2]
        a[3] = None
    return a, v


def _search(session, kind, a, v):
    et = _KINDS[kind][0]
    return _select(session, {"a": a, "v": v},
                   {"a": DType.list_(et), "v": et},
                   p=col("a").array_position(col("v")),
                   r=col("a").array_remove(col("v")))


def _same(got, want, *ctx):
    assert got.keys() == want.keys()
    for name in want:
        assert len(got[name]) == len(want[name]), (name,) + ctx
        for r, (g, w) in enumerate(zip(got[name], want[name])):
            assert repr(g) == repr(w), (name, r) + ctx


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [5, 8, 9, 16, 29, 32, 33, 64, 65, 130])
@pytest.mark.parametrize("kind", list(_KINDS))
def test_gpu_search_lane_group_widths(kind, max_len, gpu_session,
                                      cpu_session):
    """The lane group width (8/16/32/64) follows the mean length, so the
    longest rows take the stride loop; 203 rows are three validity words
    and a partial one."""
    a, v = _search_rows(kind, 203, max_len, max_len)
    want = _search(cpu_session, kind, a, v)
    assert want["p"][1] == max_len and want["p"][2] == max_len // 2 + 1
    hits = sum(1 for p in want["p"] if p)
    assert 203 // 4 < hits < 203 * 3 // 4
    _same(_search(gpu_session, kind, a, v), want, kind, max_len)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_gpu_search_row_counts(n, gpu_session, cpu_session):
    """Whole and partial validity words."""
    for kind in ("int64", "string"):
        a, v = _search_rows(kind, n, 12, 100 + n)
        _same(_search(gpu_session, kind, a, v),
              _search(cpu_session, kind, a, v), kind, n)


def _with_null_rows(c: Column, null_rows) -> Column:
    """The same column with some rows marked null; they keep their
    offsets range and the elements in it."""
    valid = np.ones(c.size, dtype=bool)
    valid[list(null_rows)] = False
    return Column(c.dtype, c.size, c.data, make_validity(valid), c.offsets,
                  None, c.child)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int64", "string"])
def test_gpu_null_rows_over_non_empty_ranges(kind):
    et = _KINDS[kind][0]
    dt = DType.list_(et)
    a, v = _search_rows(kind, 150, 20, 7)
    a[3] = a[1]
    null_rows = [r for r in range(150) if r % 5 == 3]
    for r in null_rows:      # the null rows own elements that would match
        if v[r] is None or v[r] not in (a[r] or []):
            a[r] = (a[r] or []) + [v[r] if v[r] is not None
                                   else _KINDS[kind][1][0]]
    host = _with_null_rows(Column.from_pylist(a, dt), null_rows)
    needle = Column.from_pylist(v, et)
    start = Column.from_pylist([1 + r % 3 for r in range(150)], I32)
    length = Column.from_pylist([r % 4 for r in range(150)], I32)
    dev = host.cuda()
    assert int(dev.offsets[4]) > int(dev.offsets[3])
    for fn, args in ((ops.array_position, (needle,)),
                     (ops.array_remove, (needle,)),
                     (ops.array_slice, (start, length))):
        want = fn(host, *args).to_pylist()
        got = fn(dev, *[x.cuda() for x in args]).cpu().to_pylist()
        assert repr(got) == repr(want), fn.__name__
        assert all(want[r] is None for r in null_rows)


def _view(big, lo, m):
    # word-aligned start keeps the validity view aligned
    return Column(big.dtype, m, big.data,
                  None if big.validity is None else big.validity[lo // 8:],
                  big.offsets[lo:lo + m + 1], None, big.child)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["double", "string"])
def test_gpu_nonzero_first_offset(kind):
    """A zero-copy row range of a larger LIST column: offsets[0] != 0 and
    the child holds elements of rows outside the range."""
    et = _KINDS[kind][0]
    dt = DType.list_(et)
    a, v = _search_rows(kind, 400, 12, 31)
    big = Column.from_pylist(a, dt).cuda()
    lo, m = 64, 200
    view = _view(big, lo, m)
    assert int(view.offsets[0].item()) > 0
    host = Column.from_pylist(a[lo:lo + m], dt)
    needle = Column.from_pylist(v[lo:lo + m], et)
    rng = np.random.default_rng(5)
    start = Column.from_pylist(
        [int(x) or 1 for x in rng.integers(-14, 15, m)], I32)
    length = Column.from_pylist([int(x) for x in rng.integers(0, 15, m)], I32)
    before = [t.clone() for t in (big.offsets, big.child.data)]
    for fn, args in ((ops.array_position, (needle,)),
                     (ops.array_remove, (needle,)),
                     (ops.array_slice, (start, length))):
        want = fn(host, *args).to_pylist()
        got = fn(view, *[x.cuda() for x in args]).cpu().to_pylist()
        assert repr(got) == repr(want), fn.__name__
    for x, y in zip(before, (big.offsets, big.child.data)):
        # inputs are never modified (bytes, so that a NaN equals itself)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def _slice_frame(kind, n, max_len, seed):
    rng = np.random.default_rng(seed)
    a = [None if rng.random() < 0.05 else
         _elems(kind, rng, int(rng.integers(0, max_len + 1)))
         for _ in range(n)]
    a[0] = _elems(kind, rng, max_len)
    s = [None if rng.random() < 0.05 else
         int(rng.integers(-max_len - 2, max_len + 3)) or 1 for _ in range(n)]
    ln = [None if rng.random() < 0.05 else
          int(rng.integers(0, max_len + 3)) for _ in range(n)]
    return {"a": a, "s": s, "n": ln}


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [9, 70])
@pytest.mark.parametrize("kind", ["int64", "double", "string"])
def test_gpu_slice_column_operands(kind, max_len, gpu_session, cpu_session):
    data = _slice_frame(kind, 1500, max_len, max_len)
    et = _KINDS[kind][0]
    dts = {"a": DType.list_(et), "s": I32, "n": I32}
    exprs = dict(x=col("a").slice(col("s"), col("n")),
                 y=col("a").slice(-3, col("n")), z=col("a").slice(col("s"), 2))
    want = _select(cpu_session, data, dts, **exprs)
    assert any(w for w in want["x"]) and [] in want["x"] and None in want["x"]
    _same(_select(gpu_session, data, dts, **exprs), want, kind, max_len)


@pytest.mark.gpu
def test_gpu_slice_cases_and_int32_extremes(gpu_session):
    """Start and length at the ends of INT32: the arithmetic is 64-bit, so
    nothing wraps into the row."""
    exprs = {f"s{i}": col("a").slice(s, ln)
             for i, ((s, ln), _) in enumerate(SLICES)}
    out = _select(gpu_session, {"a": [FIVE, [9]]}, {"a": L_I64}, **exprs)
    for i, (args, want) in enumerate(SLICES):
        assert out[f"s{i}"][0] == want, args
    cols = _slice_rows(gpu_session, [FIVE] * 4, [IMAX, -(2 ** 31), IMAX, 1],
                       [IMAX, IMAX, 1, IMAX])
    assert cols == [[], [], [], FIVE]


@pytest.mark.gpu
def test_gpu_slice_errors(gpu_session):
    _check_slice_errors(gpu_session)
    # the offending row in the last, partial validity word
    for bad_s, bad_n, msg in ((0, 1, START_MSG), (1, -1, LENGTH_MSG)):
        with pytest.raises(ValueError) as ei:
            _slice_rows(gpu_session, [FIVE] * 130, [1] * 129 + [bad_s],
                        [1] * 129 + [bad_n])
        assert str(ei.value) == msg


@pytest.mark.gpu
def test_gpu_slice_errors_masked_by_null(gpu_session):
    _check_slice_errors_masked(gpu_session)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int64", "string"])
def test_gpu_array_repeat(kind, gpu_session, cpu_session):
    rng = np.random.default_rng(9)
    n = 1500
    et = _KINDS[kind][0]
    data = {"e": _elems(kind, rng, n),
            "c": [None if rng.random() < 0.1 else int(rng.integers(-1, 6))
                  for _ in range(n)]}
    dts = {"e": et, "c": I32}
    exprs = dict(x=array_repeat(col("e"), col("c")),
                 y=array_repeat(col("e"), 2), z=array_repeat(col("e"), 0))
    want = _select(cpu_session, data, dts, **exprs)
    assert None in want["x"] and [] in want["x"] and [None] * 5 in want["x"]
    _same(_select(gpu_session, data, dts, **exprs), want, kind)


@pytest.mark.gpu
def test_gpu_decimal64_scalar_needles(gpu_session):
    _check_decimal_scalar_needles(gpu_session, DType.decimal(12, 2))


@pytest.mark.gpu
def test_gpu_array_repeat_overflow(gpu_session):
    """Raised from the scan total, before anything of that size exists."""
    with pytest.raises(OverflowError):
        _select(gpu_session, {"e": [1, 2], "c": [IMAX, 1]},
                {"e": I64, "c": I32}, x=array_repeat(col("e"), col("c")))


@pytest.mark.gpu
def test_gpu_empty_inputs():
    """Zero rows, and rows that are all empty or null, never launch on an
    empty child."""
    for a in ([], [[], [], []], [None, None], [[], None, []]):
        n = len(a)
        host = Column.from_pylist(a, L_I64)
        needle = Column.from_pylist([1, None, 1][:n], I64)
        one = Column.from_pylist([1] * n, I32)
        cnt = Column.from_pylist([0, None, -1][:n], I32)
        elem = Column.from_pylist([5, None, 6][:n], I64)
        for fn, args in ((ops.array_position, (host, needle)),
                         (ops.array_remove, (host, needle)),
                         (ops.array_slice, (host, one, one)),
                         (ops.array_repeat, (elem, cnt))):
            want = fn(*args)
            got = fn(*[x.cuda() for x in args]).cpu()
            assert got.dtype == want.dtype and got.size == n
            assert got.to_pylist() == want.to_pylist(), (fn.__name__, a)


@pytest.mark.gpu
def test_gpu_remaining_element_types(gpu_session, cpu_session):
    """The narrower and the logical fixed-width types take the same kernels
    with their own key transform; decimal128 only moves through the
    gather of slice and array_repeat."""
    rng = np.random.default_rng(17)
    kinds = {
        "bool": (DType.bool_(), [True, False]),
        "int8": (DType.int8(), [-128, 127, 0, -1, 5]),
        "int16": (DType.int16(), [-2 ** 15, 2 ** 15 - 1, 0, 300]),
        "float32": (DType.float32(), [NAN, -0.0, 0.0, INF, 1.5, -2.5]),
        "date": (DType.date32(), [-1, 0, 10957, 19000]),
        "timestamp": (DType.timestamp(), [-1, 0, 946684800000000, 9]),
        "decimal64": (DType.decimal(12, 2), [D("-99.50"), D("0"),
                                             D("12345.67"), D("0.01")]),
        "decimal128": (DType.decimal(30, 2), [D("2.50"), D("-1.25"),
                                              D("12345678901234567890.12")]),
    }
    for kind, (et, pool) in kinds.items():
        def pick():
            return None if rng.random() < 0.1 else \
                pool[int(rng.integers(0, len(pool)))]
        a = [None] + [[pick() for _ in range(ln)]
                      for ln in (0, 1, 3, 5, 9, 70, 300)]
        n = len(a)
        data = {"a": a, "v": [pick() for _ in range(n)],
                "s": [1, 1, -1, 2, -9, 3, 60, -299],
                "n": [2, None, 0, 1, 3, 9, 2, 400],
                "c": [2, None, 0, 1, 3, -1, 2, 4]}
        dts = {"a": DType.list_(et), "v": et, "s": I32, "n": I32, "c": I32}
        exprs = dict(s=col("a").slice(col("s"), col("n")),
                     t=array_repeat(col("v"), col("c")))
        if kind != "decimal128":
            exprs.update(p=col("a").array_position(col("v")),
                         r=col("a").array_remove(col("v")))
        tree = _frame(gpu_session, data, dts).select(
            *[e.alias(k) for k, e in exprs.items()]) \
            .physical_plan().tree_string()
        assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
        _same(_select(gpu_session, data, dts, **exprs),
              _select(cpu_session, data, dts, **exprs), kind)


@pytest.mark.gpu
def test_gpu_plan_placement_and_sql(gpu_session, cpu_session):
    data = {"a": A, "v": V, "s": [1, 2, -1, 1, -3, 1],
            "n": [2, 1, 0, None, 1, 5]}
    dts = {"a": L_I64, "v": I64, "s": I32, "n": I32}
    q = ("SELECT array_position(a, v) AS p, array_remove(a, 2) AS r, "
         "slice(a, s, n) AS s1, array_repeat(v, n) AS t, "
         "array_position(array_remove(slice(a, 1, 3), v), 2) AS nest FROM t")
    out = []
    for s in (gpu_session, cpu_session):
        s.register("t", _frame(s, data, dts))
        out.append(s.sql(q).to_pydict())
    assert out[0] == out[1]
    tree = gpu_session.sql(q).physical_plan().tree_string()
    assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
