"""array(), concat over arrays, flatten, sequence and array_join.

Both backends are new, so neither is the other's oracle: every expectation
is a literal or is computed in plain python here (the _py_* functions).
Every comparison is exact.
"""
import decimal
import os
import struct

import numpy as np
import pytest
import torch

from spark_rapids_amd import (Column, DType, array, array_join, col,
                              collect_list, flatten, lit, sequence)
from spark_rapids_amd import ops
from spark_rapids_amd.column import make_validity, mask_nbytes
from spark_rapids_amd.plan.overrides import Tagger
from spark_rapids_amd.types import DATE32

NAN = float("nan")
I32, I64, F64, STR, BOOL = (DType.int32(), DType.int64(), DType.float64(),
                            DType.string(), DType.bool_())
DATE = DATE32
D128 = DType.decimal(30, 2)
L = DType.list_
IMAX = 2 ** 31 - 1


def _frame(session, data, dtypes):
    return session.create_dataframe(data, dtypes=dtypes)


def _select(session, data, dtypes, **exprs):
    df = _frame(session, data, dtypes)
    return df.select(*[e.alias(k) for k, e in exprs.items()]).to_pydict()


def _bits(v):
    """Values with floats as their bit patterns, so that NaN equals itself
    and -0.0 differs from 0.0."""
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, (list, tuple)):
        return [_bits(x) for x in v]
    return v


# plain-python expectations ---------------------------------------------------

def _py_array(*cols):
    return [list(r) for r in zip(*cols)]


def _py_concat(*cols):
    return [None if any(p is None for p in parts)
            else [e for p in parts for e in p] for parts in zip(*cols)]


def _py_flatten(rows):
    return [None if v is None or any(p is None for p in v)
            else [e for p in v for e in p] for v in rows]


def _py_sequence(a, b, s=None):
    if a is None or b is None:
        return None
    if s is None:
        s = 1 if a <= b else -1
    if a == b:
        return [a]
    return list(range(a, b + (1 if s > 0 else -1), s))


def _py_join(rows, d, r=None):
    out = []
    for v in rows:
        if v is None:
            out.append(None)
            continue
        parts = [r if e is None else e for e in v]
        out.append(d.join(p for p in parts if p is not None))
    return out


# ---------------------------------------------------------------------------
# the literal cases of the semantics, on either backend
# ---------------------------------------------------------------------------

def _check_array(session):
    data = {"a": [1, None, 7], "b": [None, None, 8], "s": ["x", None, ""]}
    dts = {"a": I32, "b": I32, "s": STR}
    out = _select(session, data, dts, lits=array(1, None, 3),
                  cols=array(col("a"), col("b")), one=array(col("a")),
                  mixed=array(col("a"), 5, col("b"), lit(None)),
                  strs=array(col("s"), lit("k"), col("s")))
    assert out["lits"] == [[1, None, 3]] * 3
    assert out["cols"] == [[1, None], [None, None], [7, 8]]  # never NULL
    assert out["one"] == [[1], [None], [7]]
    assert out["mixed"] == [[1, 5, None, None], [None, 5, None, None],
                            [7, 5, 8, None]]
    assert out["strs"] == [["x", "k", "x"], [None, "k", None], ["", "k", ""]]


def _check_concat(session):
    data = {"x": [[1, None], None, [], [5]], "y": [[], [9], [], None],
            "z": [[2], [3], [], [6]],
            "s": [["a"], [], None, ["", None]], "t": [["b", "c"], [], ["q"], []]}
    dts = {"x": L(I32), "y": L(I32), "z": L(I32), "s": L(STR), "t": L(STR)}
    out = _select(session, data, dts,
                  three=col("x").concat(col("y")).concat(col("z")),
                  two=col("y").concat(col("z")),
                  strs=col("s").concat(col("t")))
    assert out["three"] == [[1, None, 2], None, [], None]
    assert out["two"] == [[2], [9, 3], [], None]
    assert out["strs"] == [["a", "b", "c"], [], None, ["", None]]


def _check_flatten(session):
    data = {"n": [[[1], [], [None, 2]], [[1], None], None, [], [[], []]],
            "s": [[["a", None], ["b"]], [[""]], [None], [], None]}
    out = _select(session, data, {"n": L(L(I32)), "s": L(L(STR))},
                  f=flatten(col("n")), g=col("s").flatten())
    assert out["f"] == [[1, None, 2], None, None, [], []]
    assert out["g"] == [["a", None, "b"], [""], None, [], None]


def _check_sequence(session):
    data = {"a": [1, 5, 3, None, 2], "b": [5, 1, 3, 4, None],
            "s": [2, -2, 0, 1, 1], "w": [10, 20, 30, 40, 50]}
    dts = {"a": I32, "b": I32, "s": I32, "w": I64}
    out = _select(session, data, dts, up=sequence(1, 5), down=sequence(5, 1),
                  by3=sequence(1, 10, 3), same=sequence(3, 3, 0),
                  cols=sequence(col("a"), col("b")),
                  stepped=sequence(col("a"), col("b"), col("s")),
                  wide=sequence(col("w"), 52, 20))
    assert out["up"] == [[1, 2, 3, 4, 5]] * 5
    assert out["down"] == [[5, 4, 3, 2, 1]] * 5
    assert out["by3"] == [[1, 4, 7, 10]] * 5
    assert out["same"] == [[3]] * 5
    assert out["cols"] == [[1, 2, 3, 4, 5], [5, 4, 3, 2, 1], [3], None, None]
    assert out["stepped"] == [[1, 3, 5], [5, 3, 1], [3], None, None]
    assert out["wide"] == [[10, 30, 50], [20, 40], [30, 50], [40], [50]]


def _check_sequence_extremes(session):
    lo64, hi64, lo32 = -2 ** 63, 2 ** 63 - 1, -2 ** 31
    out = _select(session, {"a": [lo64, hi64], "b": [hi64, lo64],
                            "s": [2 ** 62, -2 ** 62],
                            "c": [lo32, IMAX], "d": [IMAX, lo32],
                            "t": [2 ** 30, -2 ** 30]},
                  {"a": I64, "b": I64, "s": I64, "c": I32, "d": I32, "t": I32},
                  w=sequence(col("a"), col("b"), col("s")),
                  n=sequence(col("c"), col("d"), col("t")))
    assert out["w"] == [[lo64, lo64 + 2 ** 62, 0, 2 ** 62],
                        [hi64, hi64 - 2 ** 62, -1, -1 - 2 ** 62]]
    assert out["n"] == [[lo32, lo32 + 2 ** 30, 0, 2 ** 30],
                        [IMAX, IMAX - 2 ** 30, -1, -1 - 2 ** 30]]


def _check_sequence_errors(session):
    dts = {"a": I64, "b": I64, "s": I64}

    def run(a, b, s):
        return _select(session, {"a": a, "b": b, "s": s}, dts,
                       q=sequence(col("a"), col("b"), col("s")))["q"]

    # a zero step, a step against an ascending and against a descending
    # range; the first bad row is reported, rows masked by a NULL are not
    for rows, text in (
            (([1, 4, 9], [1, 7, 2], [0, 0, 0]), "4 to 7 by 0"),
            (([1, None, 2, 3], [3, 1, 9, 8], [1, -1, -3, -1]), "2 to 9 by -3"),
            (([5, 6, 7], [5, 2, 1], [1, 2, 1]), "6 to 2 by 2")):
        with pytest.raises(ValueError) as ex:
            run(*rows)
        assert str(ex.value) == f"Illegal sequence boundaries: {text}"
    # a legal batch after an illegal one
    assert run([1, 9], [3, 7], [1, -2]) == [[1, 2, 3], [9, 7]]
    with pytest.raises(OverflowError):
        run([0, 0], [2 ** 31 - 2, 5], [1, 1])
    with pytest.raises(OverflowError):
        run([-2 ** 63], [2 ** 63 - 1], [1])


def _check_array_join(session):
    data = {"s": [["a", None, "b"], [None, None], [], None, ["", "x", ""],
                  [None, "é"]]}
    out = _select(session, data, {"s": L(STR)}, skip=array_join(col("s"), ","),
                  repl=col("s").array_join(",", "x"),
                  nodelim=array_join(col("s"), ""),
                  wide=array_join(col("s"), "<->", ""))
    assert out["skip"] == ["a,b", "", "", None, ",x,", "é"]
    assert out["repl"] == ["a,x,b", "x,x", "", None, ",x,", "x,é"]
    assert out["nodelim"] == ["ab", "", "", None, "x", "é"]
    assert out["wide"] == ["a<-><->b", "<->", "", None, "<->x<->", "<->é"]


def _check_string_concat(session):
    """concat over strings is what it was before arrays joined in."""
    data = {"s": ["ab", None, "", "x"], "t": ["c", "d", "", None]}
    dts = {"s": STR, "t": STR}
    out = _select(session, data, dts, st=col("s").concat(col("t")),
                  lit_=col("s").concat(lit("-")).concat(col("t")))
    assert out["st"] == ["abc", None, "", None]
    assert out["lit_"] == ["ab-c", None, "-", None]
    session.register("strs", _frame(session, data, dts))
    got = session.sql("SELECT concat(s, '-', t) AS c, concat(s, t) AS d "
                      "FROM strs").to_pydict()
    assert got == {"c": ["ab-c", None, "-", None],
                   "d": ["abc", None, "", None]}


SQL_DATA = {"a": [1, None, 4], "b": [2, 3, None], "x": [[1, None], None, []],
            "y": [[], [9], [7]], "n": [[[1], [2, None]], [[3], None], []],
            "s": [["a", None, "b"], None, [None]], "k": [3, 1, 2]}
SQL_DTS = {"a": I32, "b": I32, "x": L(I32), "y": L(I32), "n": L(L(I32)),
           "s": L(STR), "k": I32}
SQL_TEXT = ("SELECT array(a, b, 7) AS arr, concat(x, y, x) AS cc, "
            "flatten(n) AS fl, sequence(1, k) AS sq, sequence(k, -2, -2) AS sd, "
            "array_join(s, ',') AS j, array_join(s, '-', 'N') AS jn FROM t")
SQL_WANT = {"arr": [[1, 2, 7], [None, 3, 7], [4, None, 7]],
            "cc": [[1, None, 1, None], None, [7]],
            "fl": [[1, 2, None], None, []],
            "sq": [[1, 2, 3], [1], [1, 2]],
            "sd": [[3, 1, -1], [1, -1], [2, 0, -2]],
            "j": ["a,b", None, ""], "jn": ["a-N-b", None, "N"]}


def _check_sql(session):
    session.register("t", _frame(session, SQL_DATA, SQL_DTS))
    assert session.sql(SQL_TEXT).to_pydict() == SQL_WANT


_CHECKS = [_check_array, _check_concat, _check_flatten, _check_sequence,
           _check_sequence_extremes, _check_sequence_errors,
           _check_array_join, _check_string_concat, _check_sql]


@pytest.mark.parametrize("check", _CHECKS, ids=lambda f: f.__name__[7:])
def test_cpu(check, cpu_session):
    check(cpu_session)


@pytest.mark.gpu
@pytest.mark.parametrize("check", _CHECKS, ids=lambda f: f.__name__[7:])
def test_gpu(check, gpu_session):
    check(gpu_session)


# ---------------------------------------------------------------------------
# types, names, tagging, docs
# ---------------------------------------------------------------------------

def test_types_and_errors(cpu_session):
    df = _frame(cpu_session, {"a": [1], "w": [1], "x": [[1]], "v": [[1]],
                              "s": [["a"]], "n": [[[1]]]},
                {"a": I32, "w": I64, "x": L(I32), "v": L(I64), "s": L(STR),
                 "n": L(L(I32))})
    sch = df.schema
    assert array(col("a"), 2).dtype(sch) == L(I32)
    assert col("x").concat(col("x")).dtype(sch) == L(I32)
    assert flatten(col("n")).dtype(sch) == L(I32)
    assert sequence(col("a"), 5).dtype(sch) == L(I32)
    assert sequence(col("w"), 5).dtype(sch) == L(I64)  # the int follows w
    assert array_join(col("s"), ",").dtype(sch) == STR
    assert not array(col("a")).nullable(sch)
    for bad in (array(col("a"), col("w")),         # no implicit widening
                array(col("a"), "x"),
                array(lit(None)),
                col("x").concat(col("v")),
                col("x").concat(col("a")),
                flatten(col("x")),
                sequence(col("a"), col("w")),
                sequence(col("a"), 2 ** 40),
                sequence(lit(1.5), 3),
                array_join(col("x"), ",")):
        with pytest.raises(TypeError):
            bad.dtype(sch)
    with pytest.raises(TypeError):
        array_join(col("s"), col("a"))
    with pytest.raises(TypeError):
        sequence(1.5, 2)
    with pytest.raises(ValueError):
        array()
    assert str(array(col("a"), 2)) == "array(a, 2)"
    assert str(flatten(col("n"))) == "flatten(n)"
    assert str(sequence(col("a"), 5, 2)) == "sequence(a, 5, 2)"
    assert str(array_join(col("s"), ",", "x")) == "array_join(s, ',', 'x')"


def test_sql_argument_count(cpu_session):
    cpu_session.register("t", _frame(cpu_session, SQL_DATA, SQL_DTS))
    for text in ("array()", "flatten(n, n)", "sequence(a)",
                 "sequence(a, b, a, b)", "array_join(s)",
                 "array_join(s, ',', 'x', 'y')"):
        with pytest.raises(ValueError):
            cpu_session.sql(f"SELECT {text} FROM t")


def _five():
    return {"CreateArray": array(col("a"), col("b")),
            "ArrayConcat": col("x").concat(col("y")),
            "Flatten": flatten(col("n")),
            "Sequence": sequence(col("a"), col("b")),
            "ArrayJoin": array_join(col("s"), ",")}


def test_tagging(session):
    sch = _frame(session, SQL_DATA, SQL_DTS).schema
    t = Tagger(session.conf)
    for name, e in _five().items():
        assert t.expr_reasons(e, sch) == [], name
    # string concat and decimal128 elements stay on the GPU
    d = _frame(session, {"d": [decimal.Decimal("1.50")], "p": ["x"]},
               {"d": D128, "p": STR}).schema
    assert t.expr_reasons(array(col("d"), col("d")), d) == []
    assert t.expr_reasons(col("p").concat(col("p")), d) == []
    for e, word in ((array(col("x"), col("y")), "array"),
                    (col("n").concat(col("n")), "concat"),
                    (flatten(array(col("n"))), "flatten")):
        reasons = t.expr_reasons(e, sch)
        assert f"{word} over nested elements on CPU" in reasons, reasons
    for name, e in _five().items():
        conf = session.conf.copy()
        conf.set(f"spark.rapids.sql.expression.{name}", False)
        assert Tagger(conf).expr_reasons(e, sch) == \
            [f"expression {name} disabled by conf"], name


def test_docgen_lists_the_functions(tmp_path, monkeypatch):
    from spark_rapids_amd.tools import docgen

    monkeypatch.setattr(docgen, "REPO", str(tmp_path))
    docgen.main()
    text = open(os.path.join(str(tmp_path), "docs",
                             "supported_ops.md")).read()
    rows = {ln.split("|")[1].strip(): ln.split("|")[3].strip()
            for ln in text.splitlines() if ln.startswith("| ")}
    for name in ("CreateArray", "ArrayConcat", "Flatten", "Sequence",
                 "ArrayJoin"):
        assert rows.get(name) == "GPU", (name, rows.get(name))


# ---------------------------------------------------------------------------
# GPU: shapes at which the kernels can go wrong
# ---------------------------------------------------------------------------

_WORDS = ["", "a", "ab", "commonprefix", "é", "zz", "-", ","]


def _values(kind, rng, m, nulls=True):
    """m python values of an element type, about a fifth of them None."""
    if kind == "int32":
        v = [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, m)]
    elif kind == "int64":
        v = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, m)]
    elif kind == "float64":
        pool = [NAN, -0.0, 0.0, float("inf"), 1.5, -2.5]
        v = [pool[int(x)] for x in rng.integers(0, len(pool), m)]
    elif kind == "bool":
        v = [bool(x) for x in rng.integers(0, 2, m)]
    elif kind == "date":
        v = [int(x) for x in rng.integers(-30000, 30000, m)]
    elif kind == "decimal128":
        v = [decimal.Decimal(int(x)) * 10 ** 14 + decimal.Decimal("0.25")
             for x in rng.integers(-2 ** 40, 2 ** 40, m)]
    else:
        v = [_WORDS[int(x)] for x in rng.integers(0, len(_WORDS), m)]
    if nulls:
        v = [None if rng.integers(0, 5) == 0 else x for x in v]
    return v


_TYPES = {"int32": I32, "int64": I64, "float64": F64, "bool": BOOL,
          "date": DATE, "decimal128": D128, "string": STR}


def _lists(kind, rng, n, max_len, null_rows=True):
    rows = []
    for _ in range(n):
        if null_rows and rng.integers(0, 7) == 0:
            rows.append(None)
        else:
            rows.append(_values(kind, rng, int(rng.integers(0, max_len + 1))))
    return rows


def _dev(values, dt):
    return Column.from_pylist(values, dt).cuda()


def _well_formed(c: Column):
    """What the existing list kernels expect of a LIST column."""
    assert c.offsets.dtype == torch.int32 and c.offsets.numel() >= c.size + 1
    offs = c.offsets[:c.size + 1].cpu().numpy()
    assert (np.diff(offs) >= 0).all()
    if c.size:
        assert c.child.size == int(offs[-1]) - int(offs[0]) or \
            c.child.size >= int(offs[-1])
    if c.validity is not None:
        assert c.validity.dtype == torch.uint8
        assert c.validity.numel() >= mask_nbytes(c.size)
        assert c.validity.data_ptr() % 8 == 0
    if c.child.validity is not None:
        assert c.child.validity.data_ptr() % 8 == 0


def _all_five(kind, n, max_len, seed):
    """Run the five ops on device columns of n rows; compare with python."""
    rng = np.random.default_rng(seed)
    dt = _TYPES[kind]
    cols = [_values(kind, rng, n) for _ in range(3)]
    got = ops.create_array([_dev(c, dt) for c in cols])
    _well_formed(got)
    assert _bits(got.cpu().to_pylist()) == _bits(_py_array(*cols)), "array"
    assert got.null_count == 0
    lists = [_lists(kind, rng, n, max_len) for _ in range(3)]
    got = ops.array_concat([_dev(x, L(dt)) for x in lists])
    _well_formed(got)
    assert _bits(got.cpu().to_pylist()) == _bits(_py_concat(*lists)), "concat"
    nested = [None if rng.integers(0, 9) == 0 else
              _lists(kind, rng, int(rng.integers(0, 4)), max_len)
              for _ in range(n)]
    got = ops.array_flatten(_dev(nested, L(L(dt))))
    _well_formed(got)
    assert _bits(got.cpu().to_pylist()) == _bits(_py_flatten(nested)), \
        "flatten"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_gpu_row_counts(n):
    """Whole and partial validity words, more than one block."""
    for kind in ("int64", "string"):
        _all_five(kind, n, 5, 10 + n)
    rng = np.random.default_rng(n)
    a = _values("int32", rng, n)
    a = [None if x is None else x % 50 for x in a]
    b = [None if rng.integers(0, 6) == 0 else int(x)
         for x in rng.integers(-20, 70, n)]
    got = ops.sequence(_dev(a, I32), _dev(b, I32))
    _well_formed(got)
    assert got.cpu().to_pylist() == [_py_sequence(x, y) for x, y in zip(a, b)]
    strs = _lists("string", rng, n, 6)
    for r in (None, "NULL"):
        got = ops.array_join(_dev(strs, L(STR)), ", ", r)
        assert got.cpu().to_pylist() == _py_join(strs, ", ", r)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(_TYPES))
def test_gpu_element_types(kind):
    """Every element type moves through unchanged, bit for bit."""
    _all_five(kind, 70, 4, 5)


_LENGTHS = [0, 1, 63, 64, 65, 2, 3000, 3, 0, 7]


@pytest.mark.gpu
def test_gpu_row_lengths():
    """Rows of 0, 1, 63, 64, 65 elements and one of 3 000 among short
    ones."""
    rng = np.random.default_rng(3)
    for kind in ("int32", "string"):
        dt = _TYPES[kind]
        a = [_values(kind, rng, m) for m in _LENGTHS]
        b = [_values(kind, rng, m) for m in reversed(_LENGTHS)]
        got = ops.array_concat([_dev(a, L(dt)), _dev(b, L(dt))])
        assert got.cpu().to_pylist() == _py_concat(a, b), kind
        # the same lengths as the number of inner arrays and as their length
        nested = [[_values(kind, rng, 2) for _ in range(m)] for m in _LENGTHS]
        nested += [[_values(kind, rng, m) for m in _LENGTHS], None]
        nested[2][40] = None           # a null inner array in a long row
        got = ops.array_flatten(_dev(nested, L(L(dt))))
        assert got.cpu().to_pylist() == _py_flatten(nested), kind
    strs = [_values("string", rng, m) for m in _LENGTHS]
    strs[6][0] = None                  # the long row opens with a skipped null
    for d, r in ((",", None), ("", None), ("--", "?"), (",", "")):
        got = ops.array_join(_dev(strs, L(STR)), d, r)
        assert got.cpu().to_pylist() == _py_join(strs, d, r), (d, r)
    start = [5] * len(_LENGTHS)
    stop = [5 + m - 1 if m else None for m in _LENGTHS]
    got = ops.sequence(_dev(start, I64), _dev(stop, I64))
    assert got.cpu().to_pylist() == \
        [_py_sequence(x, y) for x, y in zip(start, stop)]
    stop = [5 - 3 * (m - 1) if m else None for m in _LENGTHS]
    got = ops.sequence(_dev(start, I64), _dev(stop, I64),
                       _dev([-3] * len(_LENGTHS), I64))
    assert got.cpu().to_pylist() == \
        [_py_sequence(x, y, -3) for x, y in zip(start, stop)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 17])
def test_gpu_array_operand_counts(k):
    """One, two and three launches of the interleave kernel."""
    rng = np.random.default_rng(k)
    for kind, n in (("int32", 130), ("bool", 67), ("string", 40)):
        cols = [_values(kind, rng, n, nulls=j % 3 != 1) for j in range(k)]
        got = ops.create_array([_dev(c, _TYPES[kind]) for c in cols])
        _well_formed(got)
        assert got.cpu().to_pylist() == _py_array(*cols), kind
        assert got.offsets.cpu().tolist() == list(range(0, n * k + 1, k))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 9])
def test_gpu_array_mask_bits(k):
    """65 rows of alternating nulls: the child's validity words straddle
    rows and operands (and launches for k = 9) and match bit for bit."""
    n = 65
    cols = [[(i * 10 + j) if (i + j) % 2 else None for i in range(n)]
            for j in range(k)]
    got = ops.create_array([_dev(c, I64) for c in cols])
    want = np.array([(i + j) % 2 == 1 for i in range(n) for j in range(k)])
    mask = got.child.validity.cpu().numpy()
    packed = np.packbits(want.astype(np.uint8), bitorder="little")
    assert mask.size >= mask_nbytes(n * k)
    assert (mask[:packed.size] == packed).all()
    assert got.cpu().to_pylist() == _py_array(*cols)


@pytest.mark.gpu
def test_gpu_concat_nine_operands():
    rng = np.random.default_rng(9)
    for kind in ("int64", "string"):
        lists = [_lists(kind, rng, 150, 4, null_rows=j == 4)
                 for j in range(9)]
        got = ops.array_concat([_dev(x, L(_TYPES[kind])) for x in lists])
        _well_formed(got)
        assert got.cpu().to_pylist() == _py_concat(*lists), kind


def _view(big: Column, lo: int, m: int) -> Column:
    """A zero-copy row range of a LIST column (lo on a validity word)."""
    return Column(big.dtype, m, big.data,
                  None if big.validity is None else big.validity[lo // 8:],
                  big.offsets[lo:lo + m + 1], None, big.child)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["float64", "string"])
def test_gpu_sliced_inputs(kind):
    """offsets[0] != 0 in every list operand, and in the inner lists."""
    rng = np.random.default_rng(21)
    dt = _TYPES[kind]
    lo, m = 128, 150
    a, b = (_lists(kind, rng, 300, 6) for _ in range(2))
    va, vb = (_view(_dev(x, L(dt)), lo, m) for x in (a, b))
    assert int(va.offsets[0]) > 0 and int(vb.offsets[0]) > 0
    got = ops.array_concat([va, vb, va])
    want = _py_concat(a[lo:lo + m], b[lo:lo + m], a[lo:lo + m])
    assert _bits(got.cpu().to_pylist()) == _bits(want)
    nested = [None if rng.integers(0, 9) == 0 else
              _lists(kind, rng, int(rng.integers(0, 4)), 5)
              for _ in range(300)]
    big = _dev(nested, L(L(dt)))
    outer = _view(big, lo, m)                      # sliced outer
    got = ops.array_flatten(outer)
    _well_formed(got)
    assert _bits(got.cpu().to_pylist()) == _bits(_py_flatten(nested[lo:lo + m]))
    # sliced inner: the outer rows address a view of a longer inner column
    shift = int(big.offsets[lo])
    inner = _view(big.child, 64, big.child.size - 64)
    assert int(inner.offsets[0]) > 0 and shift >= 64
    outer2 = Column(big.dtype, m, big.data, outer.validity,
                    (big.offsets[lo:lo + m + 1] - 64).to(torch.int32), None,
                    inner)
    got = ops.array_flatten(outer2)
    assert _bits(got.cpu().to_pylist()) == _bits(_py_flatten(nested[lo:lo + m]))
    if kind == "string":
        for r in (None, "~"):
            got = ops.array_join(va, "+", r)
            assert got.cpu().to_pylist() == _py_join(a[lo:lo + m], "+", r)


@pytest.mark.gpu
def test_gpu_null_rows_over_non_empty_ranges():
    """A null row may own elements; they must not leak into the result."""
    rows = [["a", "b"], ["c"], ["d", None], []]
    valid = np.array([True, False, True, True])
    host = Column.from_pylist(rows, L(STR))
    c = Column(host.dtype, 4, host.data, make_validity(valid), host.offsets,
               None, host.child).cuda()
    assert ops.array_join(c, ",").cpu().to_pylist() == ["a,b", None, "d", ""]
    assert ops.array_concat([c, c]).cpu().to_pylist() == \
        [["a", "b", "a", "b"], None, ["d", None, "d", None], []]
    outer = Column.from_pylist([[["x"], ["y"]], [["z"]]], L(L(STR)))
    inner = outer.child
    inner = Column(inner.dtype, 3, inner.data,
                   make_validity(np.array([True, False, True])),
                   inner.offsets, None, inner.child)
    nested = Column(outer.dtype, 2, outer.data, None, outer.offsets, None,
                    inner).cuda()
    assert ops.array_flatten(nested).cpu().to_pylist() == [None, ["z"]]


@pytest.mark.gpu
def test_gpu_array_join_long_element():
    big = "x" * 70_000 + "é"
    rows = [["a", big, ""], [big], [None, big, None, "b"], []]
    for d, r in ((",", None), ("<>", "n/a")):
        got = ops.array_join(_dev(rows, L(STR)), d, r)
        assert got.cpu().to_pylist() == _py_join(rows, d, r)


@pytest.mark.gpu
def test_gpu_empty_and_all_empty_inputs():
    assert ops.create_array([_dev([], I32)]).cpu().to_pylist() == []
    assert ops.array_concat([_dev([], L(I32))] * 2).cpu().to_pylist() == []
    assert ops.array_flatten(_dev([], L(L(I32)))).cpu().to_pylist() == []
    assert ops.sequence(_dev([], I32), _dev([], I32)).cpu().to_pylist() == []
    assert ops.array_join(_dev([], L(STR)), ",").cpu().to_pylist() == []
    rows = [[], None, []]
    assert ops.array_concat([_dev(rows, L(I32))] * 2).cpu().to_pylist() == rows
    assert ops.array_join(_dev(rows, L(STR)), ",").cpu().to_pylist() == \
        ["", None, ""]
    assert ops.array_flatten(_dev([[], [[]], None], L(L(STR)))) \
        .cpu().to_pylist() == [[], [], None]
    assert ops.sequence(_dev([None, None], I64), _dev([1, 2], I64)) \
        .cpu().to_pylist() == [None, None]


# ---------------------------------------------------------------------------
# GPU: plan level and composition
# ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_plan_placement(gpu_session, cpu_session):
    df = _frame(gpu_session, SQL_DATA, SQL_DTS)
    five = [e.alias(k) for k, e in _five().items()]
    tree = df.select(*five).physical_plan().tree_string()
    assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
    gpu_session.register("t", df)
    tree = gpu_session.sql(SQL_TEXT).physical_plan().tree_string()
    assert "GpuProject" in tree and "cpu_bridge" not in tree, tree
    nested = array(col("x"), col("y"))
    text = df.select(nested).explain()
    assert "CpuProject[array(" in text, text
    assert "array over nested elements on CPU" in text, text
    cdf = _frame(cpu_session, SQL_DATA, SQL_DTS)
    want = [[[1, None], []], [None, [9]], [[], [7]]]
    assert list(df.select(nested).to_pydict().values()) == [want]
    assert list(cdf.select(nested).to_pydict().values()) == [want]
    for name, e in _five().items():
        off = type(gpu_session)()
        off.set("spark.rapids.sql.enabled", True)
        off.set(f"spark.rapids.sql.expression.{name}", False)
        text = _frame(off, SQL_DATA, SQL_DTS).select(e.alias("r")).explain()
        assert f"expression {name} disabled by conf" in text, text
        assert f"CpuProject[{e}" in text and f"GpuProject[{e}" not in text, \
            text


@pytest.mark.gpu
def test_gpu_and_cpu_sessions_agree_on_sql(gpu_session, cpu_session):
    out = []
    for s in (gpu_session, cpu_session):
        s.register("t", _frame(s, SQL_DATA, SQL_DTS))
        out.append(s.sql(SQL_TEXT).to_pydict())
    assert out[0] == out[1] == SQL_WANT


@pytest.mark.gpu
def test_gpu_composition(gpu_session):
    """The new columns are well-formed inputs to the existing kernels."""
    s = gpu_session
    data = {"k": [1, 2, 1, 2, 1], "s": ["a", "b", None, "d", "e"],
            "a": [1, 2, 3, 4, 5], "b": [10, None, 30, 40, 50],
            "arr": [[1], [2, 3], None, [], [4, None]], "n": [3, 0, 1, 2, 4]}
    dts = {"k": I32, "s": STR, "a": I32, "b": I32, "arr": L(I32), "n": I32}
    df = _frame(s, data, dts)
    got = df.group_by("k").agg(collect_list(col("s")).alias("l")) \
        .select(col("k"), array_join(col("l"), ",").alias("j")).to_pydict()
    assert dict(zip(got["k"], got["j"])) == {1: "a,e", 2: "b,d"}
    got = df.select(array(col("a"), col("b")).alias("p")).explode("p") \
        .to_pydict()
    assert got["p"] == [1, 10, 2, None, 3, 30, 4, 40, 5, 50]
    got = df.group_by("k").agg(collect_list(col("arr")).alias("l")) \
        .select(col("k"), flatten(col("l")).alias("f")).to_pydict()
    assert dict(zip(got["k"], got["f"])) == {1: [1, 4, None], 2: [2, 3]}
    s.register("c", df)
    got = s.sql("SELECT transform(sequence(1, n), x -> x * 2) AS t, "
                "size(array(a, b)) AS z, sort_array(concat(arr, array(a))) "
                "AS srt FROM c").to_pydict()
    assert got["t"] == [[2, 4, 6], [2, 0], [2], [2, 4], [2, 4, 6, 8]]
    assert got["z"] == [2] * 5
    assert got["srt"] == [[1, 1], [2, 2, 3], None, [4], [None, 4, 5]]
