"""Expression tree + evaluation.

The engine analogue of the reference's GpuExpression.columnarEval path
(reference: sql-plugin/src/main/scala/com/nvidia/spark/rapids/GpuExpressions.scala:139-334):
expressions evaluate batch-at-a-time to whole Columns; the same tree evaluates
on the CPU backend or on the GPU backend depending on where the batch lives.
"""
from __future__ import annotations

import decimal
import inspect
import itertools
from typing import Optional
from typing import Sequence as _Seq

import numpy as np

from ..column import Column, ColumnBatch, Field, Schema
from ..types import (BOOL, DType, FLOAT64, INT32, INT64, STRING, TypeId,
                     _adjust_decimal, as_decimal, decimal_arith_type, promote)
from .. import ops


class Expression:
    def dtype(self, schema: Schema) -> DType:
        raise NotImplementedError

    def nullable(self, schema: Schema) -> bool:
        return True

    @property
    def children(self) -> _Seq["Expression"]:
        return ()

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        raise NotImplementedError

    def output_name(self) -> str:
        return str(self)

    # ---- operator DSL --------------------------------------------------
    def _bin(self, op, other, swap=False):
        other = _as_expr(other)
        l, r = (other, self) if swap else (self, other)
        return BinaryExpr(op, l, r)

    def __add__(self, o):
        return self._bin("add", o)

    def __radd__(self, o):
        return self._bin("add", o, swap=True)

    def __sub__(self, o):
        return self._bin("sub", o)

    def __rsub__(self, o):
        return self._bin("sub", o, swap=True)

    def __mul__(self, o):
        return self._bin("mul", o)

    def __rmul__(self, o):
        return self._bin("mul", o, swap=True)

    def __truediv__(self, o):
        return self._bin("div", o)

    def __mod__(self, o):
        return self._bin("mod", o)

    def __lt__(self, o):
        return self._bin("lt", o)

    def __le__(self, o):
        return self._bin("le", o)

    def __gt__(self, o):
        return self._bin("gt", o)

    def __ge__(self, o):
        return self._bin("ge", o)

    def __eq__(self, o):  # noqa: PLE0302 - DSL
        return self._bin("eq", o)

    def __ne__(self, o):
        return self._bin("ne", o)

    def __and__(self, o):
        return self._bin("and", o)

    def __or__(self, o):
        return self._bin("or", o)

    def __invert__(self):
        return UnaryExpr("not", self)

    def __neg__(self):
        return UnaryExpr("neg", self)

    def __hash__(self):
        return id(self)

    def alias(self, name: str) -> "Alias":
        return Alias(self, name)

    def cast(self, to: DType) -> "CastExpr":
        return CastExpr(self, to)

    def is_null(self) -> "IsNull":
        return IsNull(self)

    def is_not_null(self) -> "Expression":
        return UnaryExpr("not", IsNull(self))

    # string DSL
    def contains(self, pattern: str) -> "StringPredicate":
        return StringPredicate("contains", self, pattern)

    def startswith(self, pattern: str) -> "StringPredicate":
        return StringPredicate("starts_with", self, pattern)

    def endswith(self, pattern: str) -> "StringPredicate":
        return StringPredicate("ends_with", self, pattern)

    def like(self, pattern: str) -> "StringPredicate":
        return StringPredicate("like", self, pattern)

    def rlike(self, pattern: str) -> "StringPredicate":
        """Java-regex find() semantics (RLike)."""
        return StringPredicate("rlike", self, pattern)

    def trim(self) -> "UnaryExpr":
        return UnaryExpr("trim", self)

    def ltrim(self) -> "UnaryExpr":
        return UnaryExpr("ltrim", self)

    def rtrim(self) -> "UnaryExpr":
        return UnaryExpr("rtrim", self)

    def concat(self, other) -> "BinaryExpr":
        """Spark concat(): NULL if either side is NULL. Strings join their
        bytes; arrays of one type join their elements."""
        return BinaryExpr("concat", self, _as_expr(other))

    def flatten(self) -> "Flatten":
        """The inner arrays of this array<array<T>> value as one array<T>
        (Spark flatten)."""
        return Flatten(self)

    def array_join(self, delimiter: str,
                   null_replacement: Optional[str] = None) -> "ArrayJoin":
        """The non-null strings of this array joined by `delimiter`; null
        elements are skipped, or stand as `null_replacement` (Spark
        array_join)."""
        return ArrayJoin(self, delimiter, null_replacement)

    def replace(self, search: str, replacement: str) -> "RegexpReplace":
        """Literal substring replace (StringReplace analogue), lowered to
        the regex engine with an escaped pattern."""
        esc = "".join("\\" + c if c in ".\\+*?()[]{}|^$" else c
                      for c in search)
        resc = replacement.replace("\\", "\\\\").replace("$", "\\$")
        return RegexpReplace(self, esc, resc)

    def split(self, delimiter: str) -> "StrSplit":
        """Split into a LIST of strings (java limit-0 semantics: trailing
        empty parts dropped)."""
        return StrSplit(self, delimiter)

    def element_at(self, index) -> "ElementAt":
        """1-based element of a LIST value (NULL beyond the length), or
        the value for a key of a MAP value (Spark element_at)."""
        return ElementAt(self, index)

    def size(self) -> "ArraySize":
        """Entry count of a LIST or MAP value (null -> null)."""
        return ArraySize(self)

    def array_contains(self, value) -> "ArrayContains":
        """True when the LIST value contains `value` (Spark
        array_contains; null list -> null)."""
        return ArrayContains(self, value)

    def sort_array(self, asc: bool = True) -> "SortArray":
        """Sort the elements of a LIST value (Spark sort_array): ascending
        puts nulls first, descending puts them last; NaN is greatest."""
        return SortArray(self, asc)

    def array_sort(self) -> "ArraySort":
        """Sort a LIST value ascending with nulls last (Spark array_sort,
        default comparator)."""
        return ArraySort(self)

    def array_distinct(self) -> "ArrayDistinct":
        """Drop duplicate elements of a LIST value, keeping each first
        occurrence in place (Spark array_distinct)."""
        return ArrayDistinct(self)

    def array_min(self) -> "ArrayMin":
        """Least non-null element of a LIST value (NaN greatest); NULL for
        a null, empty or all-null list."""
        return ArrayMin(self)

    def array_max(self) -> "ArrayMax":
        return ArrayMax(self)

    def array_union(self, other: "Expression") -> "ArrayUnion":
        """Distinct elements of this LIST value, then those of `other` not
        already present (Spark array_union); NULL when either is."""
        return ArrayUnion(self, other)

    def array_intersect(self, other: "Expression") -> "ArrayIntersect":
        """Distinct elements of this LIST value that also occur in `other`,
        in this value's order (Spark array_intersect)."""
        return ArrayIntersect(self, other)

    def array_except(self, other: "Expression") -> "ArrayExcept":
        """Distinct elements of this LIST value that do not occur in
        `other` (Spark array_except)."""
        return ArrayExcept(self, other)

    def arrays_overlap(self, other: "Expression") -> "ArraysOverlap":
        """True when the two LIST values share a non-null element, NULL
        when they share none, both are non-empty and either holds a null,
        else false (Spark arrays_overlap)."""
        return ArraysOverlap(self, other)

    def array_position(self, value) -> "ArrayPosition":
        """1-based place of the first element of this LIST value equal to
        `value` (an expression of the element type or a python scalar), 0
        when there is none (Spark array_position)."""
        return ArrayPosition(self, value)

    def array_remove(self, value) -> "ArrayRemove":
        """This LIST value without every element equal to `value`; null
        elements stay (Spark array_remove)."""
        return ArrayRemove(self, value)

    def slice(self, start, length) -> "ArraySlice":
        """At most `length` elements of this LIST value from the 1-based
        `start`; a negative start counts from the end (Spark slice)."""
        return ArraySlice(self, start, length)

    def transform(self, f) -> "ArrayTransform":
        """Apply `f` to every element of a LIST value (Spark transform).
        `f` is a python callable of the element, or of the element and its
        0-based position; it is called once to trace the lambda body."""
        return ArrayTransform(self, _trace_lambda("transform", f, 2))

    def filter(self, f) -> "ArrayFilter":
        """Keep the elements of a LIST value for which `f(x)` or `f(x, i)`
        is true (Spark filter)."""
        return ArrayFilter(self, _trace_lambda("filter", f, 2))

    def exists(self, f) -> "ArrayExists":
        """True when `f(x)` is true for an element of a LIST value, NULL
        when none is and one is NULL, else false (Spark exists)."""
        return ArrayExists(self, _trace_lambda("exists", f, 1))

    def forall(self, f) -> "ArrayForAll":
        """False when `f(x)` is false for an element of a LIST value, NULL
        when none is and one is NULL, else true (Spark forall)."""
        return ArrayForAll(self, _trace_lambda("forall", f, 1))

    def regexp_extract(self, pattern: str, group: int = 1) -> "RegexpExtract":
        return RegexpExtract(self, pattern, group)

    def lpad(self, width: int, fill: str = " ") -> "PadExpr":
        return PadExpr(self, width, fill, left=True)

    def rpad(self, width: int, fill: str = " ") -> "PadExpr":
        return PadExpr(self, width, fill, left=False)

    def locate(self, substr: str, pos: int = 1) -> "LocateExpr":
        """1-based position of substr (0 when absent) — Spark locate/instr."""
        return LocateExpr(self, substr, pos)

    def get_json_object(self, path: str) -> "GetJsonObject":
        return GetJsonObject(self, path)

    def json_tuple(self, *fields) -> list:
        """One expression per top-level field, aliased c0, c1, ..."""
        return json_tuple(self, *fields)

    def regexp_extract_all(self, pattern: str,
                           group: int = 1) -> "RegexpExtractAll":
        return RegexpExtractAll(self, pattern, group)

    def regexp_replace(self, pattern: str, replacement: str) -> "RegexpReplace":
        return RegexpReplace(self, pattern, replacement)

    def substr(self, pos: int, length: int = -1) -> "Substring":
        return Substring(self, pos, length)

    def length(self) -> "UnaryExpr":
        return UnaryExpr("length", self)

    def initcap(self) -> "UnaryExpr":
        """Capitalize each space-separated word (ASCII on GPU)."""
        return UnaryExpr("initcap", self)

    def reverse(self) -> "UnaryExpr":
        """Reverse codepoint order."""
        return UnaryExpr("reverse", self)

    def upper(self) -> "UnaryExpr":
        return UnaryExpr("upper", self)

    def lower(self) -> "UnaryExpr":
        return UnaryExpr("lower", self)


def _as_expr(v) -> Expression:
    if isinstance(v, Expression):
        return v
    return Literal(v)


class ColumnRef(Expression):
    def __init__(self, name: str):
        self.name = name

    def dtype(self, schema: Schema) -> DType:
        return schema.field(self.name).dtype

    def nullable(self, schema: Schema) -> bool:
        return schema.field(self.name).nullable

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return batch.columns[schema.index(self.name)]

    def output_name(self) -> str:
        return self.name

    def __str__(self):
        return self.name


def _infer_literal_dtype(v) -> DType:
    if isinstance(v, bool):
        return BOOL
    if isinstance(v, int):
        return INT32 if -(2 ** 31) <= v < 2 ** 31 else INT64
    if isinstance(v, float):
        return FLOAT64
    if isinstance(v, str):
        return STRING
    if v is None:
        return DType(TypeId.NULL)
    raise TypeError(f"unsupported literal {v!r}")


class Literal(Expression):
    def __init__(self, value, dtype: Optional[DType] = None):
        self.value = value
        self._dtype = dtype or _infer_literal_dtype(value)

    def dtype(self, schema: Schema) -> DType:
        return self._dtype

    def nullable(self, schema: Schema) -> bool:
        return self.value is None

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        if self.value is None:
            return Column.nulls(self._dtype if self._dtype.id is not TypeId.NULL
                                else INT32, batch.num_rows, batch.device)
        return Column.full(self.value, self._dtype, batch.num_rows,
                           batch.device)

    def __str__(self):
        return repr(self.value)


def _decimal_exact(lt: DType, rt: DType) -> bool:
    """True when mul/div should use exact decimal arithmetic (at least one
    decimal operand, the other decimal or integral)."""
    return (lt.is_decimal or rt.is_decimal) \
        and (lt.is_decimal or lt.is_integral) \
        and (rt.is_decimal or rt.is_integral)


# ops whose result is boolean
_BOOL_OPS = {"eq", "ne", "lt", "le", "gt", "ge", "and", "or", "eq_null_safe"}
# ops that force double output (Spark `/`)
_DOUBLE_OPS = {"div", "pow"}


class BinaryExpr(Expression):
    def __init__(self, op: str, left: Expression, right: Expression):
        self.op = op
        self.left = left
        self.right = right

    @property
    def children(self):
        return (self.left, self.right)

    def _common(self, lt: DType, rt: DType) -> DType:
        if (lt.is_decimal or rt.is_decimal) and self.op in (
                "int_div", "mod", "pmod", "pow"):
            raise NotImplementedError(
                f"decimal {self.op} needs scale arithmetic (not implemented "
                "yet): cast to double first, e.g. col.cast(FLOAT64)")
        if (lt.is_decimal or rt.is_decimal) and self.op in ("mul", "div"):
            # mixed decimal/floating (the exact-decimal path handles
            # decimal/integral): Spark casts the decimal side to double
            return FLOAT64
        if lt.id is TypeId.NULL:
            return rt
        if rt.id is TypeId.NULL:
            return lt
        if lt == rt:
            return lt
        if self.op in _DOUBLE_OPS:
            return FLOAT64
        return promote(lt, rt)

    def _in_dtype(self, schema) -> DType:
        return self._common(self.left.dtype(schema), self.right.dtype(schema))

    def _array_concat(self, schema: Schema) -> Optional["ArrayConcat"]:
        """concat is typed by its operands, which only the schema tells:
        over arrays, the whole chain of nested concats (the SQL parser
        folds concat(a, b, c) to the left) is one ArrayConcat; over
        anything else this is None and the string path below stands."""
        if self.op != "concat":
            return None
        leaves: list = []
        todo = [self]
        while todo:
            e = todo.pop()
            if isinstance(e, BinaryExpr) and e.op == "concat":
                todo += (e.right, e.left)
            else:
                leaves.append(e)
        if not any(e.dtype(schema).id is TypeId.LIST for e in leaves):
            return None
        return ArrayConcat(*leaves)

    def dtype(self, schema: Schema) -> DType:
        # NOTE: children's dtype() is called exactly once here — recursing
        # more than once makes deep expression chains exponential
        if self.op in _BOOL_OPS:
            return BOOL
        arrays = self._array_concat(schema)
        if arrays is not None:
            return arrays.dtype(schema)
        lt, rt = self.left.dtype(schema), self.right.dtype(schema)
        if self.op in ("mul", "div") and _decimal_exact(lt, rt):
            # Spark DecimalPrecision rules: scale s1+s2 (mul) /
            # max(6, s1+p2+1) (div), precision-loss adjustment at 38
            return decimal_arith_type(self.op, lt, rt)
        if self.op in _DOUBLE_OPS:
            return FLOAT64
        if self.op == "sub" and lt.is_timelike and rt.is_timelike:
            return INT32  # datediff domain
        it = self._common(lt, rt)
        if it.is_decimal and self.op in ("add", "sub"):
            # Spark add/sub result: max(p1-s1,p2-s2)+max(s1,s2)+1 at
            # scale max(s1,s2); promote() already produced the first part.
            return _adjust_decimal(it.precision + 1, it.scale)
        return it

    # ops where `scalar OP col` can run through the col-scalar kernel
    _COMMUTATIVE = {"add", "mul", "eq", "ne", "eq_null_safe", "and", "or",
                    "bitand", "bitor", "bitxor", "min", "max"}
    _SWAP_CMP = {"lt": "gt", "gt": "lt", "le": "ge", "ge": "le"}

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        arrays = self._array_concat(schema)
        if arrays is not None:
            return arrays.eval(batch, schema)
        if self.op in ("mul", "div"):
            lt, rt = self.left.dtype(schema), self.right.dtype(schema)
            if _decimal_exact(lt, rt):
                # operands keep their own scales; the backend computes the
                # exact product/quotient at the Spark result scale
                lcol = ops.cast(self.left.eval(batch, schema), as_decimal(lt))
                rcol = ops.cast(self.right.eval(batch, schema), as_decimal(rt))
                return ops.decimal_mul_div(
                    self.op, lcol, rcol, decimal_arith_type(self.op, lt, rt))
        common = self._in_dtype(schema)
        if self.op in _DOUBLE_OPS and not common.is_decimal:
            common = FLOAT64
        out = self.dtype(schema)
        if out.is_decimal and out.id is TypeId.DECIMAL128 \
                and common.id is TypeId.DECIMAL64:
            # result crosses into decimal128 (e.g. (18,0)+(18,0) -> (19,0)):
            # widen the operands so the 128-bit kernel runs end to end
            common = DType(TypeId.DECIMAL128, common.precision, common.scale)
        # scalar fast path: literal on either side
        if isinstance(self.right, Literal) and self.right.value is not None \
                and not common.is_decimal and self.op != "concat":
            lcol = ops.cast(self.left.eval(batch, schema), common)
            return ops.binary_op_scalar(self.op, lcol, _coerce_py(self.right.value, common), out)
        if isinstance(self.left, Literal) and self.left.value is not None \
                and not common.is_decimal and self.op != "concat":
            swapped = self.op if self.op in self._COMMUTATIVE \
                else self._SWAP_CMP.get(self.op)
            if swapped is not None:
                rcol = ops.cast(self.right.eval(batch, schema), common)
                return ops.binary_op_scalar(
                    swapped, rcol, _coerce_py(self.left.value, common), out)
            if self.op == "sub":
                # c - x == -(x - c): two scalar kernels, no literal column
                rcol = ops.cast(self.right.eval(batch, schema), common)
                d = ops.binary_op_scalar(
                    "sub", rcol, _coerce_py(self.left.value, common), out)
                return ops.unary_op("neg", d, out)
        lcol = ops.cast(self.left.eval(batch, schema), common)
        rcol = ops.cast(self.right.eval(batch, schema), common)
        return ops.binary_op(self.op, lcol, rcol, out)

    def __str__(self):
        return f"({self.left} {self.op} {self.right})"


def _coerce_py(v, dtype: DType):
    if dtype.is_floating:
        return float(v)
    if dtype.is_integral or dtype.is_decimal:
        return int(v)
    return v


_UNARY_OUT = {
    "not": lambda t: BOOL,
    "trim": lambda t: STRING,
    "initcap": lambda t: STRING,
    "reverse": lambda t: STRING,
    "ltrim": lambda t: STRING,
    "rtrim": lambda t: STRING,
    "is_nan": lambda t: BOOL,
    "neg": lambda t: t,
    "abs": lambda t: t,
    "sqrt": lambda t: FLOAT64,
    "exp": lambda t: FLOAT64,
    "log": lambda t: FLOAT64,
    "sin": lambda t: FLOAT64,
    "cos": lambda t: FLOAT64,
    "tan": lambda t: FLOAT64,
    "floor": lambda t: INT64 if not t.is_decimal else t,
    "ceil": lambda t: INT64 if not t.is_decimal else t,
    "length": lambda t: INT32,
    "upper": lambda t: STRING,
    "lower": lambda t: STRING,
    "year": lambda t: INT32,
    "month": lambda t: INT32,
    "day": lambda t: INT32,
}


class UnaryExpr(Expression):
    def __init__(self, op: str, child: Expression):
        self.op = op
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return _UNARY_OUT[self.op](self.child.dtype(schema))

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        if self.op in ("sqrt", "exp", "log", "sin", "cos", "tan"):
            c = ops.cast(c, FLOAT64)
        return ops.unary_op(self.op, c, self.dtype(schema))

    def __str__(self):
        return f"{self.op}({self.child})"


class IsNull(Expression):
    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return BOOL

    def nullable(self, schema: Schema) -> bool:
        return False

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.is_null(self.child.eval(batch, schema))

    def __str__(self):
        return f"isnull({self.child})"


class CastExpr(Expression):
    def __init__(self, child: Expression, to: DType):
        self.child = child
        self.to = to

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.to

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.cast(self.child.eval(batch, schema), self.to)

    def __str__(self):
        return f"cast({self.child} as {self.to})"


class Alias(Expression):
    def __init__(self, child: Expression, name: str):
        self.child = child
        self.name = name

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema)

    def nullable(self, schema: Schema) -> bool:
        return self.child.nullable(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return self.child.eval(batch, schema)

    def output_name(self) -> str:
        return self.name

    def __str__(self):
        return f"{self.child} AS {self.name}"


class CaseWhen(Expression):
    """CASE WHEN cond THEN v ... ELSE e END  (pairs of (cond, value))."""

    def __init__(self, branches, else_expr: Optional[Expression] = None):
        self.branches = [(c, _as_expr(v)) for c, v in branches]
        self.else_expr = _as_expr(else_expr) if else_expr is not None else None

    @property
    def children(self):
        out = []
        for c, v in self.branches:
            out.extend([c, v])
        if self.else_expr is not None:
            out.append(self.else_expr)
        return tuple(out)

    def dtype(self, schema: Schema) -> DType:
        t = self.branches[0][1].dtype(schema)
        for _, v in self.branches[1:]:
            vt = v.dtype(schema)
            if t.id is TypeId.NULL:
                t = vt
            elif vt.id is not TypeId.NULL:
                t = promote(t, vt)
        if self.else_expr is not None:
            et = self.else_expr.dtype(schema)
            if et.id is not TypeId.NULL:
                t = promote(t, et) if t.id is not TypeId.NULL else et
        return t

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        out_t = self.dtype(schema)
        # evaluate as nested if_else from the last branch backwards
        if self.else_expr is not None:
            acc = ops.cast(self.else_expr.eval(batch, schema), out_t)
        else:
            acc = Column.nulls(out_t, batch.num_rows, batch.device)
        backend = ops.backend_for(*batch.columns) if batch.columns else None
        for cond, val in reversed(self.branches):
            c = cond.eval(batch, schema)
            v = ops.cast(val.eval(batch, schema), out_t)
            acc = ops.backend_for(c, v, acc).if_else(c, v, acc)
        return acc

    def __str__(self):
        parts = " ".join(f"WHEN {c} THEN {v}" for c, v in self.branches)
        e = f" ELSE {self.else_expr}" if self.else_expr is not None else ""
        return f"CASE {parts}{e} END"


class StringPredicate(Expression):
    """contains / starts_with / ends_with / LIKE against a literal pattern
    (reference analogue: GpuContains/GpuStartsWith/GpuLike)."""

    def __init__(self, op: str, child: Expression, pattern: str):
        self.op = op
        self.child = child
        self.pattern = pattern

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return BOOL

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        return ops.backend_for(c).str_predicate(self.op, c, self.pattern)

    def __str__(self):
        return f"{self.op}({self.child}, {self.pattern!r})"


class Substring(Expression):
    """Spark substring(str, pos, len): 1-based pos in codepoints, negative
    pos counts from the end; len < 0 means to-the-end."""

    def __init__(self, child: Expression, pos: int, length: int = -1):
        self.child = child
        self.pos = pos
        self.length = length

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return STRING

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        return ops.backend_for(c).substring(c, self.pos, self.length)

    def __str__(self):
        return f"substring({self.child}, {self.pos}, {self.length})"


# ---------------------------------------------------------------------------
# public DSL
# ---------------------------------------------------------------------------

class StrSplit(Expression):
    """split(str, delim) -> array<string>. GPU kernel handles literal
    delimiters (k_str_split_* in strings.hip); regex delimiters run on
    the CPU via re.split (GpuStringSplit analogue)."""

    def __init__(self, child: Expression, delimiter: str):
        self.child = child
        self.delimiter = delimiter

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return DType.list_(STRING)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.str_split(self.child.eval(batch, schema), self.delimiter)

    def __str__(self):
        return f"split({self.child}, {self.delimiter!r})"


class ElementAt(Expression):
    """element_at(array, k) with 1-based k (negative k counts from the
    end); NULL when |k| exceeds the length. element_at(map, key) returns
    the value for key or NULL (GpuElementAt analogue)."""

    def __init__(self, child: Expression, index):
        self.child = child
        self.index = index

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        cdt = self.child.dtype(schema)
        return cdt.children[1] if cdt.id is TypeId.MAP else cdt.children[0]

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        if c.dtype.id is TypeId.MAP:
            return ops.map_get(c, self.index)
        assert isinstance(self.index, int) and self.index != 0, \
            "element_at(array, k) is 1-based (Spark semantics)"
        return ops.element_at(c, self.index)

    def __str__(self):
        return f"element_at({self.child}, {self.index})"


class ArrayContains(Expression):
    """array_contains(array, value) -> bool (GpuArrayContains)."""

    def __init__(self, child: Expression, value):
        self.child = child
        self.value = value

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return BOOL

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.array_contains(self.child.eval(batch, schema),
                                  self.value)

    def __str__(self):
        return f"array_contains({self.child}, {self.value!r})"


class ArraySize(Expression):
    """size(array) -> int32; null array -> null (GpuSize analogue)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return INT32

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.array_size(self.child.eval(batch, schema))

    def __str__(self):
        return f"size({self.child})"


class SortArray(Expression):
    """sort_array(array, asc): stable sort inside each list; ascending
    puts nulls first, descending last (GpuSortArray analogue)."""

    def __init__(self, child: Expression, ascending: bool = True):
        self.child = child
        self.ascending = bool(ascending)

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.sort_array(self.child.eval(batch, schema),
                              self.ascending, self.ascending)

    def __str__(self):
        return f"sort_array({self.child}, {str(self.ascending).lower()})"


class ArraySort(Expression):
    """array_sort(array): ascending, nulls last; default comparator only
    (GpuArraySort analogue)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.sort_array(self.child.eval(batch, schema), True, False)

    def __str__(self):
        return f"array_sort({self.child})"


class ArrayDistinct(Expression):
    """array_distinct(array): first occurrences in input order, at most
    one null (GpuArrayDistinct KEEP_FIRST)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.array_distinct(self.child.eval(batch, schema))

    def __str__(self):
        return f"array_distinct({self.child})"


class ArrayMin(Expression):
    """array_min(array): least non-null element, NaN greatest; NULL when
    there is none (GpuArrayMin analogue)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema).children[0]

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.array_min(self.child.eval(batch, schema))

    def __str__(self):
        return f"array_min({self.child})"


class ArrayMax(Expression):
    """array_max(array): greatest non-null element (GpuArrayMax)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema).children[0]

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.array_max(self.child.eval(batch, schema))

    def __str__(self):
        return f"array_max({self.child})"


class _ArraySetOp(Expression):
    """Two LIST operands of one element type; element equality is
    array_distinct's (NaN equals NaN, -0.0 equals 0.0, null equals null).
    A row is NULL when either operand row is."""

    fn = ""

    def __init__(self, left: Expression, right: Expression):
        self.left = left
        self.right = right

    @property
    def children(self):
        return (self.left, self.right)

    def _list_dtype(self, schema: Schema) -> DType:
        lt, rt = self.left.dtype(schema), self.right.dtype(schema)
        if lt.id is not TypeId.LIST or rt.id is not TypeId.LIST or lt != rt:
            raise TypeError(f"{self.fn} needs two arrays of the same element "
                            f"type, got {lt} and {rt}")
        return lt

    def dtype(self, schema: Schema) -> DType:
        return self._list_dtype(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._list_dtype(schema)
        return getattr(ops, self.fn)(self.left.eval(batch, schema),
                                     self.right.eval(batch, schema))

    def __str__(self):
        return f"{self.fn}({self.left}, {self.right})"


class ArrayUnion(_ArraySetOp):
    """array_union(a, b): distinct(a) then the distinct elements of b not
    in a, first-occurrence order (GpuArrayUnion analogue)."""

    fn = "array_union"


class ArrayIntersect(_ArraySetOp):
    """array_intersect(a, b): distinct elements of a that occur in b, a's
    order and bit patterns (GpuArrayIntersect analogue)."""

    fn = "array_intersect"


class ArrayExcept(_ArraySetOp):
    """array_except(a, b): distinct elements of a that do not occur in b
    (GpuArrayExcept analogue)."""

    fn = "array_except"


class ArraysOverlap(_ArraySetOp):
    """arrays_overlap(a, b): true / NULL / false, see
    Expression.arrays_overlap (GpuArraysOverlap analogue)."""

    fn = "arrays_overlap"

    def dtype(self, schema: Schema) -> DType:
        self._list_dtype(schema)
        return DType.bool_()


def _decimal_needle(fn: str, v, et: DType) -> decimal.Decimal:
    """An int, float or Decimal scalar as the Decimal VALUE it stands for,
    which Column.full then scales: 5 against decimal(12, 2) is 5.00, never
    the unscaled 0.05. There is no widening here either: a value that
    decimal(p, s) cannot hold exactly is a TypeError, not a needle that
    matches nothing."""
    ctx = decimal.Context(prec=60)
    d = decimal.Decimal(repr(v)) if isinstance(v, float) \
        else decimal.Decimal(v)
    ok = d.is_finite()
    if ok:
        unscaled = d.scaleb(et.scale, ctx)
        ok = unscaled == unscaled.to_integral_value() and \
            abs(unscaled) < 10 ** et.precision
    if not ok:
        raise TypeError(f"{fn}: the value {v!r} cannot be held exactly by "
                        f"elements of type {et}")
    return d


def _needle_literal(fn: str, v, et: DType) -> Literal:
    """A python scalar as a Literal of the element type `et`, coerced by
    value the way _coerce_py does it (an int widens to a floating element
    type; an int, a float or a Decimal stands for its value against a
    decimal one); a scalar of another kind is a TypeError."""
    if v is None:
        return Literal(None, et)
    if isinstance(v, bool):
        ok = et.id is TypeId.BOOL
    elif isinstance(v, int):
        ok = et.id is not TypeId.BOOL and (
            et.is_integral or et.is_floating or et.is_decimal
            or et.id in (TypeId.DATE32, TypeId.TIMESTAMP))
    elif isinstance(v, float):
        ok = et.is_floating or et.is_decimal
    elif isinstance(v, str):
        ok = et.id is TypeId.STRING
    elif isinstance(v, decimal.Decimal):
        ok = et.is_decimal
    else:
        ok = False
    if not ok:
        raise TypeError(f"{fn}: the {type(v).__name__} value {v!r} cannot be "
                        f"compared with elements of type {et}")
    if et.is_decimal:
        return Literal(_decimal_needle(fn, v, et), et)
    return Literal(_coerce_py(v, et), et)


class _ArrayNeedleFn(Expression):
    """A LIST value and a value `v` of exactly its element type, one per
    row: a column, a typed literal or a computed expression (no implicit
    widening, as with the set operations). Only a python scalar is coerced
    to the element type, by value; `lit(None)` is a null needle. Element
    equality is array_distinct's, except that a null element equals
    nothing. A row is NULL when the array or `v` is."""

    fn = ""

    def __init__(self, child: Expression, value):
        self.child = child
        self.value = value  # an Expression, or the python scalar as given

    @property
    def children(self):
        if isinstance(self.value, Expression):
            return (self.child, self.value)
        return (self.child,)

    def _needle(self, schema: Schema) -> Expression:
        cdt = self.child.dtype(schema)
        if cdt.id is not TypeId.LIST:
            raise TypeError(f"{self.fn} needs an array input, got {cdt}")
        et = cdt.children[0]
        v = self.value
        if not isinstance(v, Expression):
            return _needle_literal(self.fn, v, et)
        vt = v.dtype(schema)
        if vt.id is TypeId.NULL and isinstance(v, Literal):
            return Literal(None, et)
        if vt != et:
            raise TypeError(f"{self.fn} needs a value of the array's element "
                            f"type, got {cdt} and {vt}")
        return v

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        needle = self._needle(schema)
        return getattr(ops, self.fn)(self.child.eval(batch, schema),
                                     needle.eval(batch, schema))

    def __str__(self):
        v = self.value
        return f"{self.fn}({self.child}, " \
               f"{v if isinstance(v, Expression) else repr(v)})"


class ArrayPosition(_ArrayNeedleFn):
    """array_position(a, v): INT64 1-based place of the first element equal
    to v, 0 when there is none (GpuArrayPosition analogue)."""

    fn = "array_position"

    def dtype(self, schema: Schema) -> DType:
        self._needle(schema)
        return INT64


class ArrayRemove(_ArrayNeedleFn):
    """array_remove(a, v): a without every element equal to v; order, null
    elements and bit patterns are kept (GpuArrayRemove analogue)."""

    fn = "array_remove"

    def dtype(self, schema: Schema) -> DType:
        self._needle(schema)
        return self.child.dtype(schema)


def _int32_operand(fn: str, what: str, v) -> Expression:
    if isinstance(v, bool) or not isinstance(v, (int, Expression)):
        raise TypeError(f"{fn}: {what} must be an int or an integer "
                        f"expression, got {type(v).__name__}")
    if isinstance(v, int):
        if not -(2 ** 31) <= v < 2 ** 31:
            raise ValueError(f"{fn}: {what} {v} is outside the INT32 range")
        return Literal(v, INT32)
    return v


def _as_int32(fn: str, what: str, e: Expression, schema: Schema) -> Expression:
    """`e` cast to INT32 with the engine's CastExpr; integer types only."""
    t = e.dtype(schema)
    if isinstance(e, Literal) and e.value is None:
        return Literal(None, INT32)
    if not t.is_integral or t.id is TypeId.BOOL:
        raise TypeError(f"{fn}: {what} must be an integer, got {t}")
    return e if t == INT32 else CastExpr(e, INT32)


class ArraySlice(Expression):
    """slice(a, start, length): the elements from the 1-based `start` (a
    negative one counts from the end), at most `length` of them; an empty
    array when the start falls outside the row. start and length are
    python ints or integer expressions, cast to INT32. NULL when any of the
    three is; start == 0 or length < 0 in a row where none is raises
    ValueError (GpuSlice analogue)."""

    def __init__(self, child: Expression, start, length):
        self.child = child
        self.start = _int32_operand("slice", "start", start)
        self.length = _int32_operand("slice", "length", length)

    @property
    def children(self):
        return (self.child, self.start, self.length)

    def _operands(self, schema: Schema):
        cdt = self.child.dtype(schema)
        if cdt.id is not TypeId.LIST:
            raise TypeError(f"slice needs an array input, got {cdt}")
        return (_as_int32("slice", "start", self.start, schema),
                _as_int32("slice", "length", self.length, schema))

    def dtype(self, schema: Schema) -> DType:
        self._operands(schema)
        return self.child.dtype(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        start, length = self._operands(schema)
        return ops.array_slice(self.child.eval(batch, schema),
                               start.eval(batch, schema),
                               length.eval(batch, schema))

    def __str__(self):
        return f"slice({self.child}, {self.start}, {self.length})"


class ArrayRepeat(Expression):
    """array_repeat(e, n): an array of n copies of e; empty for n <= 0, NULL
    for a null n, an array of nulls for a null e. n is a python int or an
    integer expression, cast to INT32 (GpuArrayRepeat analogue)."""

    def __init__(self, child, count):
        self.child = _as_expr(child)
        self.count = _int32_operand("array_repeat", "count", count)

    @property
    def children(self):
        return (self.child, self.count)

    def _count(self, schema: Schema) -> Expression:
        return _as_int32("array_repeat", "count", self.count, schema)

    def dtype(self, schema: Schema) -> DType:
        self._count(schema)
        et = self.child.dtype(schema)
        if et.id is TypeId.NULL:
            raise TypeError("array_repeat needs a typed element; cast the "
                            "NULL literal")
        return DType.list_(et)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self.dtype(schema)
        return ops.array_repeat(self.child.eval(batch, schema),
                                self._count(schema).eval(batch, schema))

    def __str__(self):
        return f"array_repeat({self.child}, {self.count})"


def _is_null_literal(e: Expression, schema: Schema) -> bool:
    return isinstance(e, Literal) and e.value is None and \
        e.dtype(schema).id is TypeId.NULL


def _one_operand_type(fn: str, exprs, schema: Schema) -> DType:
    """The one type all of `exprs` have; an untyped NULL literal takes it.
    There is no implicit widening, as with the set operations."""
    dt = None
    for e in exprs:
        if _is_null_literal(e, schema):
            continue
        t = e.dtype(schema)
        if dt is None:
            dt = t
        elif t != dt:
            raise TypeError(f"{fn} needs operands of one type, got {dt} "
                            f"and {t}")
    if dt is None:
        raise TypeError(f"{fn} needs a typed operand; cast a NULL literal")
    return dt


def _typed_operands(exprs, dt: DType, schema: Schema):
    return [Literal(None, dt) if _is_null_literal(e, schema) else e
            for e in exprs]


class CreateArray(Expression):
    """array(e1, ..., ek): row i is [e1[i], ..., ek[i]]. The row is never
    NULL; an element is null where its operand is. All operands have
    exactly one type (GpuCreateArray analogue)."""

    def __init__(self, *exprs):
        if not exprs:
            raise ValueError("array needs at least one operand")
        self.exprs = tuple(_as_expr(e) for e in exprs)

    @property
    def children(self):
        return self.exprs

    def dtype(self, schema: Schema) -> DType:
        return DType.list_(_one_operand_type("array", self.exprs, schema))

    def nullable(self, schema: Schema) -> bool:
        return False

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        et = _one_operand_type("array", self.exprs, schema)
        return ops.create_array(
            [e.eval(batch, schema)
             for e in _typed_operands(self.exprs, et, schema)])

    def __str__(self):
        return f"array({', '.join(str(e) for e in self.exprs)})"


class ArrayConcat(Expression):
    """concat(a1, ..., ak) over arrays of exactly one type: the rows'
    elements in operand order, null elements kept; NULL when any operand
    row is (GpuConcat analogue). `concat` over values whose types are only
    known with the schema is a BinaryExpr, which hands its LIST case here."""

    def __init__(self, *exprs):
        if not exprs:
            raise ValueError("concat needs at least one operand")
        self.exprs = tuple(_as_expr(e) for e in exprs)

    @property
    def children(self):
        return self.exprs

    def dtype(self, schema: Schema) -> DType:
        dt = _one_operand_type("concat", self.exprs, schema)
        if dt.id is not TypeId.LIST:
            raise TypeError(f"concat over arrays got {dt}")
        return dt

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        dt = self.dtype(schema)
        return ops.array_concat(
            [e.eval(batch, schema)
             for e in _typed_operands(self.exprs, dt, schema)])

    def __str__(self):
        return f"concat({', '.join(str(e) for e in self.exprs)})"


class Flatten(Expression):
    """flatten(a) for a : array<array<T>>: the row's inner arrays in order
    as one array<T>; NULL when the row or any inner array of it is
    (GpuFlatten analogue)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        cdt = self.child.dtype(schema)
        if cdt.id is not TypeId.LIST or \
                cdt.children[0].id is not TypeId.LIST:
            raise TypeError(f"flatten needs an array of arrays, got {cdt}")
        return cdt.children[0]

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self.dtype(schema)
        return ops.array_flatten(self.child.eval(batch, schema))

    def __str__(self):
        return f"flatten({self.child})"


def _sequence_operand(what: str, v) -> Expression:
    if isinstance(v, bool) or not isinstance(v, (int, Expression)):
        raise TypeError(f"sequence: {what} must be an int or an integer "
                        f"expression, got {type(v).__name__}")
    return _as_expr(v)


class Sequence(Expression):
    """sequence(start, stop[, step]): start, start + step, ... up to stop,
    all INT32 or all INT64. Without a step it is 1 where start <= stop, else
    -1. NULL when any operand is. start == stop gives [start] whatever the
    step; otherwise a zero step, or one pointing away from stop, raises
    ValueError (GpuSequence analogue; dates and timestamps are not
    covered)."""

    def __init__(self, start, stop, step=None):
        self.start = _sequence_operand("start", start)
        self.stop = _sequence_operand("stop", stop)
        self.step = None if step is None else _sequence_operand("step", step)

    @property
    def children(self):
        return tuple(e for e in (self.start, self.stop, self.step)
                     if e is not None)

    def _operands(self, schema: Schema):
        """The operands at their one type. A python int given next to an
        INT64 operand was inferred as INT32 by its value alone, so it takes
        the other operands' type; expressions are never cast."""
        exprs = list(self.children)
        typed = [e.dtype(schema) for e in exprs
                 if not isinstance(e, Literal)]
        if typed and all(t == typed[0] for t in typed) and \
                typed[0].id in (TypeId.INT32, TypeId.INT64):
            exprs = [Literal(e.value, typed[0])
                     if isinstance(e, Literal) and
                     (e.value is None or e.dtype(schema).is_integral)
                     else e for e in exprs]
        dt = _one_operand_type("sequence", exprs, schema)
        if dt.id not in (TypeId.INT32, TypeId.INT64):
            raise TypeError(f"sequence needs INT32 or INT64 operands, got "
                            f"{dt}")
        for e in exprs:
            if isinstance(e, Literal) and e.value is not None and \
                    dt.id is TypeId.INT32 and \
                    not -(2 ** 31) <= e.value < 2 ** 31:
                raise TypeError(f"sequence: {e.value} is outside INT32")
        exprs = _typed_operands(exprs, dt, schema)
        return dt, exprs[0], exprs[1], (exprs[2] if len(exprs) > 2 else None)

    def dtype(self, schema: Schema) -> DType:
        return DType.list_(self._operands(schema)[0])

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        _, start, stop, step = self._operands(schema)
        return ops.sequence(start.eval(batch, schema),
                            stop.eval(batch, schema),
                            None if step is None
                            else step.eval(batch, schema))

    def __str__(self):
        return "sequence(" + ", ".join(str(e) for e in self.children) + ")"


class ArrayJoin(Expression):
    """array_join(a, delimiter[, null_replacement]) for a : array<string>:
    the non-null elements joined by the delimiter; null elements are
    skipped, or stand as the replacement when one is given. The delimiter
    and the replacement are string literals. NULL when the array is
    (GpuArrayJoin analogue)."""

    def __init__(self, child: Expression, delimiter: str,
                 null_replacement: Optional[str] = None):
        for what, v in (("delimiter", delimiter),
                        ("null replacement", null_replacement)):
            if isinstance(v, Literal):
                v = v.value
            if not isinstance(v, str) and \
                    not (v is None and what != "delimiter"):
                raise TypeError(f"array_join: the {what} must be a string "
                                f"literal, got {type(v).__name__}")
        self.child = child
        self.delimiter = delimiter.value if isinstance(delimiter, Literal) \
            else delimiter
        self.null_replacement = null_replacement.value \
            if isinstance(null_replacement, Literal) else null_replacement

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        cdt = self.child.dtype(schema)
        if cdt.id is not TypeId.LIST or \
                cdt.children[0].id is not TypeId.STRING:
            raise TypeError(f"array_join needs an array of strings, got "
                            f"{cdt}")
        return STRING

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self.dtype(schema)
        return ops.array_join(self.child.eval(batch, schema), self.delimiter,
                              self.null_replacement)

    def __str__(self):
        r = "" if self.null_replacement is None \
            else f", {self.null_replacement!r}"
        return f"array_join({self.child}, {self.delimiter!r}{r})"


class _StringDigest(Expression):
    """A function of one STRING operand's UTF-8 bytes (what Spark's implicit
    string-to-binary cast hashes; there is no BINARY type). NULL where the
    operand is. Any other operand type is a TypeError from dtype(), as
    Spark rejects it at analysis time."""

    fn = ""

    def __init__(self, child):
        self.child = _as_expr(child)

    @property
    def children(self):
        return (self.child,)

    def _check(self, schema: Schema):
        cdt = self.child.dtype(schema)
        if cdt.id is not TypeId.STRING:
            raise TypeError(f"{self.fn} needs a string input, got {cdt}")

    def dtype(self, schema: Schema) -> DType:
        self._check(schema)
        return STRING

    def __str__(self):
        return f"{self.fn}({self.child})"


class Md5(_StringDigest):
    """md5(s): 32 lowercase hex digits (GpuMd5 analogue)."""

    fn = "md5"

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._check(schema)
        return ops.digest_hex(self.child.eval(batch, schema), "md5")


class Sha1(_StringDigest):
    """sha1(s) / sha(s): 40 lowercase hex digits (GpuSha1 analogue)."""

    fn = "sha1"

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._check(schema)
        return ops.digest_hex(self.child.eval(batch, schema), "sha1")


class Sha2(_StringDigest):
    """sha2(s, bits): the SHA-2 digest of that many bits as lowercase hex.
    bits is an int literal; 0 means 256; anything but 0, 224, 256, 384 and
    512 gives NULL in every row, as in Spark (GpuSha2 analogue)."""

    fn = "sha2"
    _ALGO = {0: "sha256", 224: "sha224", 256: "sha256", 384: "sha384",
             512: "sha512"}

    def __init__(self, child, bits):
        super().__init__(child)
        if isinstance(bits, Literal):
            bits = bits.value
        if isinstance(bits, bool) or not isinstance(bits, int):
            raise ValueError(f"sha2: the bit length must be an int literal, "
                             f"got {bits}")
        self.bits = bits

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._check(schema)
        algo = self._ALGO.get(self.bits)
        if algo is None:
            return Column.nulls(STRING, batch.num_rows, batch.device)
        return ops.digest_hex(self.child.eval(batch, schema), algo)

    def __str__(self):
        return f"sha2({self.child}, {self.bits})"


class Crc32(_StringDigest):
    """crc32(s): the zlib CRC-32 as an unsigned value in a BIGINT (GpuCrc32
    analogue)."""

    fn = "crc32"

    def dtype(self, schema: Schema) -> DType:
        self._check(schema)
        return INT64

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._check(schema)
        return ops.crc32(self.child.eval(batch, schema))


# what murmur3_hash and xxhash64 hash in both backends today
_ROW_HASH_TYPES = (TypeId.BOOL, TypeId.INT8, TypeId.INT16, TypeId.INT32,
                   TypeId.DATE32, TypeId.INT64, TypeId.TIMESTAMP,
                   TypeId.DECIMAL64, TypeId.FLOAT32, TypeId.FLOAT64,
                   TypeId.STRING)


class _RowHash(Expression):
    """A seed-42 hash of one or more operands, chained column by column. A
    NULL operand leaves the running hash as it is, so the result is never
    NULL."""

    fn = ""

    def __init__(self, *exprs):
        if not exprs:
            raise ValueError(f"{self.fn} takes at least one argument")
        self.exprs = [_as_expr(e) for e in exprs]

    @property
    def children(self):
        return tuple(self.exprs)

    def _check(self, schema: Schema):
        for e in self.exprs:
            dt = e.dtype(schema)
            if dt.id not in _ROW_HASH_TYPES:
                raise TypeError(f"{self.fn} over {dt} operands is not "
                                "supported")

    def nullable(self, schema: Schema) -> bool:
        return False

    def __str__(self):
        return f"{self.fn}(" + ", ".join(str(e) for e in self.exprs) + ")"


class Murmur3Hash(_RowHash):
    """hash(e1, ..., ek): Spark's murmur3_x86_32 row hash, INT32
    (GpuMurmur3Hash analogue)."""

    fn = "hash"

    def dtype(self, schema: Schema) -> DType:
        self._check(schema)
        return INT32

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._check(schema)
        return ops.murmur3_hash([e.eval(batch, schema) for e in self.exprs],
                                42)


class XxHash64(_RowHash):
    """xxhash64(e1, ..., ek): canonical XXH64 row hash, INT64 (GpuXxHash64
    analogue)."""

    fn = "xxhash64"

    def dtype(self, schema: Schema) -> DType:
        self._check(schema)
        return INT64

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        self._check(schema)
        return ops.xxhash64([e.eval(batch, schema) for e in self.exprs], 42)


_lambda_ids = itertools.count()


class LambdaVariable(Expression):
    """An argument of a lambda: the element `x` or its 0-based position `i`.
    Deliberately not a ColumnRef, so column pruning never mistakes it for a
    column of the input. `column` is the unique name it goes by in the
    element schema, which keeps it apart from an outer column of the same
    name and from the `x` of a sibling lambda."""

    def __init__(self, name: str):
        self.name = name
        self.column = f"{name}#{next(_lambda_ids)}"

    def dtype(self, schema: Schema) -> DType:
        return schema.field(self.column).dtype

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return batch.columns[schema.index(self.column)]

    def output_name(self) -> str:
        return self.name

    def __str__(self):
        return self.name


class LambdaFunction(Expression):
    """`x -> body` or `(x, i) -> body`; typed and evaluated against the
    element schema of the higher-order function that owns it."""

    def __init__(self, args: _Seq[LambdaVariable], body: Expression):
        self.args = tuple(args)
        self.body = body

    @property
    def children(self):
        return (self.body,)

    def dtype(self, schema: Schema) -> DType:
        return self.body.dtype(schema)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return self.body.eval(batch, schema)

    def __str__(self):
        names = ", ".join(a.name for a in self.args)
        return f"{names if len(self.args) == 1 else f'({names})'} -> " \
               f"{self.body}"


def _free_lambda_vars(e: Expression) -> list:
    """LambdaVariables under `e` that no LambdaFunction under `e` binds."""
    if isinstance(e, LambdaVariable):
        return [e]
    if isinstance(e, LambdaFunction):
        return [v for v in _free_lambda_vars(e.body)
                if not any(v is a for a in e.args)]
    return [v for c in e.children for v in _free_lambda_vars(c)]


def _outer_refs(e: Expression, out: set) -> set:
    if isinstance(e, ColumnRef):
        out.add(e.name)
    for c in e.children:
        _outer_refs(c, out)
    return out


class _ArrayLambda(Expression):
    """A LIST value and a lambda over its elements (reference analogue:
    GpuArrayTransform / GpuArrayFilter / GpuArrayExists). The body is an
    ordinary projection over the flattened child: one row per element,
    holding the element, its position when the lambda names it, and the
    outer columns the body refers to, gathered by the element-to-row map."""

    fn = ""
    max_args = 1
    predicate = True

    def __init__(self, child: Expression, function: LambdaFunction):
        if not isinstance(function, LambdaFunction):
            raise TypeError(f"{self.fn} needs a lambda, got "
                            f"{type(function).__name__}")
        if not 1 <= len(function.args) <= self.max_args:
            raise ValueError(
                f"{self.fn} takes a lambda of "
                f"{'one argument' if self.max_args == 1 else 'one or two arguments'}"
                f", got {len(function.args)}")
        free = [v for v in _free_lambda_vars(function.body)
                if not any(v is a for a in function.args)]
        if free:
            raise NotImplementedError(
                f"{self.fn}: a lambda nested in the body of another lambda "
                f"cannot refer to the outer lambda's variable {free[0]}")
        self.child = child
        self.function = function

    @property
    def children(self):
        return (self.child, self.function)

    def _var_fields(self, schema: Schema) -> list:
        cdt = self.child.dtype(schema)
        if cdt.id is not TypeId.LIST:
            raise TypeError(f"{self.fn} needs an array input, got {cdt}")
        args = self.function.args
        return [Field(args[0].column, cdt.children[0])] + \
            [Field(a.column, INT32, False) for a in args[1:]]

    def element_schema(self, schema: Schema) -> Schema:
        """The schema the body is typed against: the outer schema plus the
        lambda variables."""
        return Schema(list(schema.fields) + self._var_fields(schema))

    def _body_dtype(self, schema: Schema) -> DType:
        bt = self.function.dtype(self.element_schema(schema))
        if self.predicate and bt.id is not TypeId.BOOL:
            raise TypeError(f"{self.fn} needs a boolean lambda body, got {bt}")
        return bt

    def _finish(self, arr: Column, res: Column, span) -> Column:
        raise NotImplementedError

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        bt = self._body_dtype(schema)
        arr = self.child.eval(batch, schema)
        span = off0, total = ops.list_span(arr)
        if total == 0:
            # nothing to evaluate the body on: an empty column of its type
            return self._finish(
                arr, Column.from_pylist([], bt).to(arr.device), span)
        body = self.function.body
        args = self.function.args
        used = _free_lambda_vars(body)
        elems = arr.child
        if off0 != 0 or total != elems.size:
            idx = Column.from_numpy(
                np.arange(off0, off0 + total, dtype=np.int32),
                device=arr.device)
            elems = ops.gather(ColumnBatch([elems], elems.size), idx,
                               negatives=False).columns[0]
        names = _outer_refs(body, set())
        outer = [f for f in schema.fields if f.name in names]
        with_pos = len(args) > 1 and any(v is args[1] for v in used)
        fields = self._var_fields(schema)[:2 if with_pos else 1]
        cols = [elems]
        if outer or with_pos:
            rowid, pos = ops.list_element_rows(arr, with_pos, span)
            if with_pos:
                cols.append(pos)
            if outer:
                src = ColumnBatch([batch.columns[schema.index(f.name)]
                                   for f in outer], batch.num_rows)
                cols += ops.gather(src, rowid, negatives=False).columns
                fields += outer
        res = body.eval(ColumnBatch(cols, total), Schema(fields))
        return self._finish(arr, res, span)

    def __str__(self):
        return f"{self.fn}({self.child}, {self.function})"


class ArrayTransform(_ArrayLambda):
    """transform(a, x -> f) / transform(a, (x, i) -> f): the body's value
    for every element; offsets and row validity are the input's."""

    fn = "transform"
    max_args = 2
    predicate = False

    def dtype(self, schema: Schema) -> DType:
        return DType.list_(self._body_dtype(schema))

    def _finish(self, arr: Column, res: Column, span) -> Column:
        n = arr.size
        offs = arr.offsets[:n + 1]
        if span[0]:
            offs = ops.binary_op_scalar(
                "sub", Column(INT32, n + 1, offs, None, null_count=0),
                span[0], INT32).data
        return Column(DType.list_(res.dtype), n, arr.data, arr.validity, offs,
                      arr._null_count, res)


class ArrayFilter(_ArrayLambda):
    """filter(a, x -> p) / filter(a, (x, i) -> p): the elements whose
    predicate is true, order kept; false and NULL drop the element."""

    fn = "filter"
    max_args = 2

    def dtype(self, schema: Schema) -> DType:
        self._body_dtype(schema)
        return self.child.dtype(schema)

    def _finish(self, arr: Column, res: Column, span) -> Column:
        return ops.array_filter(arr, res, span)


class ArrayExists(_ArrayLambda):
    """exists(a, x -> p), three-valued: true if any predicate is true, else
    NULL if any is NULL, else false."""

    fn = "exists"

    def dtype(self, schema: Schema) -> DType:
        self._body_dtype(schema)
        return BOOL

    def _finish(self, arr: Column, res: Column, span) -> Column:
        return ops.array_exists(arr, res, span)


class ArrayForAll(_ArrayLambda):
    """forall(a, x -> p): false if any predicate is false, else NULL if any
    is NULL, else true."""

    fn = "forall"

    def dtype(self, schema: Schema) -> DType:
        self._body_dtype(schema)
        return BOOL

    def _finish(self, arr: Column, res: Column, span) -> Column:
        return ops.array_forall(arr, res, span)


def _trace_lambda(fn: str, f, max_args: int) -> LambdaFunction:
    """Call the python callable `f` once with LambdaVariables named after
    its parameters and take what it returns as the lambda body."""
    if isinstance(f, LambdaFunction):
        return f
    if not callable(f):
        raise TypeError(f"{fn} needs a callable, got {type(f).__name__}")
    try:
        params = list(inspect.signature(f).parameters.values())
    except (TypeError, ValueError) as ex:
        raise TypeError(f"{fn}: cannot read the callable's signature: {ex}")
    plain = (inspect.Parameter.POSITIONAL_ONLY,
             inspect.Parameter.POSITIONAL_OR_KEYWORD)
    if not 1 <= len(params) <= max_args or \
            any(p.kind not in plain for p in params):
        raise ValueError(
            f"{fn} takes a callable of "
            f"{'one argument' if max_args == 1 else 'one or two arguments'}"
            f", got {inspect.signature(f)}")
    args = [LambdaVariable(p.name) for p in params]
    body = f(*args)
    if not isinstance(body, (Expression, bool, int, float, str)):
        raise TypeError(f"{fn}: the callable returned "
                        f"{type(body).__name__}, not an expression")
    return LambdaFunction(args, _as_expr(body))


def transform(a, f) -> ArrayTransform:
    """transform(a, lambda x: ...) or transform(a, lambda x, i: ...)."""
    return _as_expr(a).transform(f)


def filter_(a, f) -> ArrayFilter:
    """filter(a, lambda x: ...) or filter(a, lambda x, i: ...)."""
    return _as_expr(a).filter(f)


def exists(a, f) -> ArrayExists:
    return _as_expr(a).exists(f)


def forall(a, f) -> ArrayForAll:
    return _as_expr(a).forall(f)


def array_position(a, v) -> ArrayPosition:
    return _as_expr(a).array_position(v)


def array_remove(a, v) -> ArrayRemove:
    return _as_expr(a).array_remove(v)


def slice_(a, start, length) -> ArraySlice:
    """slice(a, start, length); the underscore keeps python's slice."""
    return _as_expr(a).slice(start, length)


def array_repeat(e, count) -> ArrayRepeat:
    return ArrayRepeat(e, count)


def array(*exprs) -> CreateArray:
    return CreateArray(*exprs)


def flatten(a) -> Flatten:
    return _as_expr(a).flatten()


def sequence(start, stop, step=None) -> Sequence:
    return Sequence(start, stop, step)


def array_join(a, delimiter: str,
               null_replacement: Optional[str] = None) -> ArrayJoin:
    return _as_expr(a).array_join(delimiter, null_replacement)


def md5(e) -> Md5:
    return Md5(e)


def sha1(e) -> Sha1:
    return Sha1(e)


def sha2(e, bits: int) -> Sha2:
    return Sha2(e, bits)


def crc32(e) -> Crc32:
    return Crc32(e)


def hash_(*exprs) -> Murmur3Hash:
    """hash(e1, ..., ek); the underscore keeps python's hash."""
    return Murmur3Hash(*exprs)


def xxhash64(*exprs) -> XxHash64:
    return XxHash64(*exprs)


class HostStringFn(Expression):
    """A scalar string function evaluated on the host (rows through a
    python callable); the overrides pass tags it off the GPU, so inside a
    GPU project it executes via CpuBridge. Used for the long tail of
    string builtins (repeat, substring_index, translate, ...) until they
    earn kernels."""

    def __init__(self, name: str, child: Expression, fn, out_dtype=None):
        self.name = name
        self.child = child
        self.fn = fn
        self._out = out_dtype or STRING

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self._out

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        host = c if not c.is_cuda else c.cpu()
        out = [None if v is None else self.fn(v) for v in host.to_pylist()]
        res = Column.from_pylist(out, self._out)
        return res.cuda() if c.is_cuda else res

    def __str__(self):
        return f"{self.name}({self.child})"


def repeat_str(e, n: int) -> HostStringFn:
    return HostStringFn("repeat", _as_expr(e), lambda v: v * n)


def substring_index(e, delim: str, count: int) -> HostStringFn:
    """Spark substring_index: text before the count-th delimiter
    (negative count: after the count-th from the right)."""

    def fn(v, d=delim, c=count):
        parts = v.split(d)
        if c > 0:
            return d.join(parts[:c])
        if c < 0:
            return d.join(parts[c:])
        return ""

    return HostStringFn("substring_index", _as_expr(e), fn)


def translate(e, src: str, repl: str) -> HostStringFn:
    table = {ord(a): (repl[i] if i < len(repl) else None)
             for i, a in enumerate(src)}
    return HostStringFn("translate", _as_expr(e),
                        lambda v: v.translate(table))


def ascii_(e) -> HostStringFn:
    return HostStringFn("ascii", _as_expr(e),
                        lambda v: ord(v[0]) if v else 0, INT32)


class PadExpr(Expression):
    """lpad/rpad to a fixed width (GpuStringLPad/RPad analogue; CPU
    evaluation this round — tagged off the GPU by the overrides pass)."""

    def __init__(self, child: Expression, width: int, fill: str, left: bool):
        self.child = child
        self.width = width
        # empty fill is meaningful (Spark UTF8String.lpad: empty pad just
        # truncates to width); only None defaults to a space
        self.fill = " " if fill is None else fill
        self.left = left

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return STRING

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        return ops.str_pad(c, self.width, self.fill, self.left)

    def __str__(self):
        side = "lpad" if self.left else "rpad"
        return f"{side}({self.child}, {self.width}, {self.fill!r})"


class LocateExpr(Expression):
    """locate(substr, str, pos): 1-based find, 0 when absent (GpuLocate)."""

    def __init__(self, child: Expression, substr: str, pos: int = 1):
        self.child = child
        self.substr = substr
        self.pos = pos

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return INT32

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        return ops.str_locate(c, self.substr, self.pos)

    def __str__(self):
        return f"locate({self.substr!r}, {self.child}, {self.pos})"


class ConcatWs(Expression):
    """concat_ws(sep, c1, c2, ...): join non-null values with sep; rows
    with every value null give "" (never NULL — Spark concat_ws)."""

    def __init__(self, sep: str, *exprs: Expression):
        self.sep = sep
        self.exprs = [_as_expr(e) for e in exprs]

    @property
    def children(self):
        return tuple(self.exprs)

    def dtype(self, schema: Schema) -> DType:
        return STRING

    def nullable(self, schema: Schema) -> bool:
        return False

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        cols = [e.eval(batch, schema) for e in self.exprs]
        return ops.concat_ws(self.sep, cols)

    def __str__(self):
        args = ", ".join(str(e) for e in self.exprs)
        return f"concat_ws({self.sep!r}, {args})"


def concat_ws(sep: str, *exprs) -> ConcatWs:
    return ConcatWs(sep, *exprs)


class GetJsonObject(Expression):
    """get_json_object(col, path): path is `$` followed by `.name`,
    `['name']` and `[n]` steps (expr/json_path.py). On the GPU a validating
    per-row JSON parser with a path matcher (json.hip) answers nested keys,
    array indexes, escaped strings and object/array results itself, and
    hands single rows whose host rendering it cannot reproduce (e.g. a float
    spelt `1e2`) to the CPU json parser. Wildcards raise; a malformed path
    gives NULL on every row (GpuGetJsonObject analogue).

    A GPU project that holds several of these over one child parses each row
    once for all of them (ProjectExec) and leaves the columns in the batch's
    memo, from which eval() takes its own."""

    def __init__(self, child: Expression, path: str):
        from . import json_path

        self.child = child
        self.path = path
        # None for a malformed path; raises for a wildcard
        self.steps = json_path.parse(path)
        self.text = None

    @classmethod
    def from_steps(cls, child: Expression, steps, text: str):
        """The same expression for a path given as parsed steps (None: a
        malformed path), which may hold key names that no path string can
        spell. `text` is how the node prints."""
        node = cls.__new__(cls)
        node.child = child
        node.path = None
        node.steps = None if steps is None else list(steps)
        node.text = text
        return node

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return STRING

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        if batch.memo is not None:
            fused = batch.memo.get(id(self))
            if fused is not None:
                return fused
        child = self.child.eval(batch, schema)
        if self.path is None:
            return ops.get_json_object_multi(child, [self.steps])[0]
        return ops.get_json_object(child, self.path)

    def __str__(self):
        if self.path is None:
            return self.text
        return f"get_json_object({self.child}, {self.path!r})"


def json_tuple(e, *fields) -> list:
    """json_tuple(e, f0, f1, ...): the top-level fields f0, f1, ... of the
    JSON object in `e`, as expressions aliased c0, c1, ... Field i is
    get_json_object with the single key step fields[i]: the name is a literal
    key, never a path, so `a.b`, `x[0]`, `it's` and the empty string name
    members. A None field gives NULL on every row (GpuJsonTuple analogue)."""
    from . import json_path

    if not fields:
        raise ValueError("json_tuple needs at least one field")
    child = _as_expr(e)
    out = []
    for i, f in enumerate(fields):
        if f is not None and not isinstance(f, str):
            raise TypeError("json_tuple fields are strings or None")
        steps = None if f is None else [(json_path.KEY, f)]
        node = GetJsonObject.from_steps(
            child, steps, f"json_tuple({child}, {f!r})")
        out.append(Alias(node, f"c{i}"))
    return out


class CpuBridge(Expression):
    """Evaluate a CPU-only expression inside a GPU projection via a host
    round-trip, so one unsupported expression no longer demotes the whole
    project (reference analogue: GpuCpuBridgeExpression /
    GpuCpuBridgeOptimizer)."""

    def __init__(self, child: Expression):
        self.child = child

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return self.child.dtype(schema)

    def nullable(self, schema: Schema) -> bool:
        return self.child.nullable(schema)

    def output_name(self) -> str:
        return self.child.output_name()

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        if batch.columns and batch.columns[0].is_cuda:
            out = self.child.eval(batch.cpu(), schema)
            return out.cuda()
        return self.child.eval(batch, schema)

    def __str__(self):
        return f"cpu_bridge({self.child})"


class RegexpExtract(Expression):
    """regexp_extract(str, pattern, idx): the capture group's text for the
    first match; "" when no match or non-participating group (Spark
    semantics). GPU: capture-group backtracking VM (regex.hip k_regex_extract);
    reference analogue: GpuRegExpExtract over the transpiled cudf regex."""

    def __init__(self, child: Expression, pattern: str, group: int = 1):
        self.child = child
        self.pattern = pattern
        self.group = group

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return STRING

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.regexp_extract(self.child.eval(batch, schema),
                                  self.pattern, self.group)

    def __str__(self):
        return f"regexp_extract({self.child}, {self.pattern!r}, {self.group})"


class RegexpExtractAll(Expression):
    """regexp_extract_all: every match's group text as array<string>
    (GpuRegExpExtractAll analogue; shares the capture-group VM)."""

    def __init__(self, child: Expression, pattern: str, group: int = 1):
        self.child = child
        self.pattern = pattern
        self.group = group

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return DType.list_(STRING)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.regexp_extract_all(self.child.eval(batch, schema),
                                      self.pattern, self.group)

    def __str__(self):
        return (f"regexp_extract_all({self.child}, {self.pattern!r}, "
                f"{self.group})")


class RegexpReplace(Expression):
    """regexp_replace(str, pattern, replacement) with $g group references
    (GpuRegExpReplace analogue; java Matcher.appendReplacement semantics
    incl. empty-match advancement)."""

    def __init__(self, child: Expression, pattern: str, replacement: str):
        self.child = child
        self.pattern = pattern
        self.replacement = replacement

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        return STRING

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        return ops.regexp_replace(self.child.eval(batch, schema),
                                  self.pattern, self.replacement)

    def __str__(self):
        return (f"regexp_replace({self.child}, {self.pattern!r}, "
                f"{self.replacement!r})")


class Coalesce(Expression):
    def __init__(self, *exprs):
        self.exprs = [_as_expr(e) for e in exprs]

    @property
    def children(self):
        return tuple(self.exprs)

    def dtype(self, schema: Schema) -> DType:
        t = self.exprs[0].dtype(schema)
        for e in self.exprs[1:]:
            et = e.dtype(schema)
            if t.id is TypeId.NULL:
                t = et
            elif et.id is not TypeId.NULL and et != t:
                t = promote(t, et)
        return t

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        out_t = self.dtype(schema)
        acc = ops.cast(self.exprs[-1].eval(batch, schema), out_t)
        for e in reversed(self.exprs[:-1]):
            c = ops.cast(e.eval(batch, schema), out_t)
            acc = ops.backend_for(c, acc).if_else(_not_null(c), c, acc)
        return acc

    def __str__(self):
        return f"coalesce({', '.join(str(e) for e in self.exprs)})"


def _not_null(c: Column) -> Column:
    return ops.unary_op("not", ops.is_null(c), BOOL)


class Round(Expression):
    """Spark round(): HALF_UP at `scale` decimal places."""

    def __init__(self, child, scale: int = 0):
        self.child = _as_expr(child)
        self.scale = scale

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        t = self.child.dtype(schema)
        return t if t.is_decimal or t.is_integral else FLOAT64

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        t = self.child.dtype(schema)
        c = self.child.eval(batch, schema)
        if t.is_integral and self.scale >= 0:
            return c
        if t.is_decimal:
            shift = t.scale - self.scale
            if shift <= 0:
                return c
            rescaled = ops.cast(c, DType.decimal(t.precision, self.scale))
            return ops.cast(rescaled, t)
        c = ops.cast(c, FLOAT64)
        return ops.backend_for(c).round_half_up(c, self.scale)

    def __str__(self):
        return f"round({self.child}, {self.scale})"


def col(name: str) -> ColumnRef:
    return ColumnRef(name)


def lit(v, dtype: Optional[DType] = None) -> Literal:
    return Literal(v, dtype)


def when(cond: Expression, value) -> CaseWhen:
    return CaseWhen([(cond, value)])


def coalesce(*exprs) -> Coalesce:
    return Coalesce(*exprs)


def round_(e, scale: int = 0) -> Round:
    return Round(e, scale)


def _null_aware_fold(op: str, exprs):
    """greatest/least: Spark skips NULLs (result null only if all null)."""
    es = [_as_expr(e) for e in exprs]
    acc = es[0]
    for e in es[1:]:
        pick = BinaryExpr(op, acc, e)
        acc = CaseWhen([(IsNull(acc), e), (IsNull(e), acc)], pick)
    return acc


def greatest(*exprs) -> Expression:
    return _null_aware_fold("max", exprs)


def least(*exprs) -> Expression:
    return _null_aware_fold("min", exprs)


def isin(e, *values) -> Expression:
    e = _as_expr(e)
    acc = BinaryExpr("eq", e, Literal(values[0]))
    for v in values[1:]:
        acc = BinaryExpr("or", acc, BinaryExpr("eq", e, Literal(v)))
    return acc


def hour(ts) -> Expression:
    """hour of a timestamp (micros since epoch, UTC)."""
    e = _as_expr(ts)
    return BinaryExpr("pmod", BinaryExpr("int_div", CastExpr(e, INT64),
                                         Literal(3_600_000_000)),
                      Literal(24))


def minute(ts) -> Expression:
    e = _as_expr(ts)
    return BinaryExpr("pmod", BinaryExpr("int_div", CastExpr(e, INT64),
                                         Literal(60_000_000)), Literal(60))


def second(ts) -> Expression:
    e = _as_expr(ts)
    return BinaryExpr("pmod", BinaryExpr("int_div", CastExpr(e, INT64),
                                         Literal(1_000_000)), Literal(60))


def date_add(d, days) -> Expression:
    return BinaryExpr("add", _as_expr(d), _as_expr(days))


def date_sub(d, days) -> Expression:
    return BinaryExpr("sub", _as_expr(d), _as_expr(days))


def to_date(ts) -> Expression:
    """timestamp (micros) -> date32 days, floored for pre-epoch values."""
    e = _as_expr(ts)
    us = CastExpr(e, INT64)
    rem = BinaryExpr("pmod", us, Literal(86_400_000_000))
    days = BinaryExpr("int_div", BinaryExpr("sub", us, rem),
                      Literal(86_400_000_000))
    return CastExpr(days, DType.date32())


def unix_timestamp(ts) -> Expression:
    """timestamp -> whole seconds since epoch (floored)."""
    e = _as_expr(ts)
    us = CastExpr(e, INT64)
    rem = BinaryExpr("pmod", us, Literal(1_000_000))
    return BinaryExpr("int_div", BinaryExpr("sub", us, rem),
                      Literal(1_000_000))


def dayofweek(d) -> Expression:
    """Spark dayofweek: 1 = Sunday .. 7 = Saturday (1970-01-01 was a
    Thursday, day-number 4 in this scheme)."""
    e = _as_expr(d)
    days = CastExpr(CastExpr(e, DType.date32()), INT64)
    return BinaryExpr("add",
                      BinaryExpr("pmod", BinaryExpr("add", days,
                                                    Literal(4)),
                                 Literal(7)), Literal(1))


def quarter(d) -> Expression:
    """quarter 1..4 from the month."""
    e = _as_expr(d)
    m = UnaryExpr("month", e)
    return BinaryExpr("add",
                      BinaryExpr("int_div",
                                 BinaryExpr("sub", m, Literal(1)),
                                 Literal(3)), Literal(1))


def datediff(end, start) -> Expression:
    from ..types import DATE32

    return BinaryExpr("sub", CastExpr(_as_expr(end), DATE32),
                      CastExpr(_as_expr(start), DATE32))


class CreateNamedStruct(Expression):
    """named_struct(n1, e1, n2, e2, ...) -> STRUCT column (reference
    analogue: GpuCreateNamedStruct). The struct itself is never null."""

    def __init__(self, names, exprs):
        self.names = list(names)
        self.exprs = [_as_expr(e) for e in exprs]

    @property
    def children(self):
        return tuple(self.exprs)

    def dtype(self, schema: Schema) -> DType:
        return DType.struct_(
            [(n, e.dtype(schema)) for n, e in zip(self.names, self.exprs)])

    def nullable(self, schema: Schema) -> bool:
        return False

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        import torch

        kids = tuple(e.eval(batch, schema) for e in self.exprs)
        dev = kids[0].device if kids else batch.device
        return Column(self.dtype(schema), batch.num_rows,
                      torch.zeros(0, dtype=torch.uint8, device=dev),
                      None, None, 0, kids)

    def output_name(self) -> str:
        return "named_struct(" + ", ".join(self.names) + ")"

    def __str__(self):
        inner = ", ".join(f"{n}: {e}" for n, e in
                          zip(self.names, self.exprs))
        return f"named_struct({inner})"


class GetStructField(Expression):
    """struct.field access (reference analogue: GpuGetStructField)."""

    def __init__(self, child, name: str):
        self.child = _as_expr(child)
        self.name = name

    @property
    def children(self):
        return (self.child,)

    def _field_index(self, schema) -> int:
        st = self.child.dtype(schema)
        if st.id is not TypeId.STRUCT:
            raise TypeError(f"getField on non-struct {st}")
        if self.name not in st.field_names:
            raise KeyError(
                f"struct has no field {self.name!r} (has "
                f"{list(st.field_names)})")
        return st.field_names.index(self.name)

    def dtype(self, schema: Schema) -> DType:
        st = self.child.dtype(schema)
        return st.children[self._field_index(schema)]

    def nullable(self, schema: Schema) -> bool:
        return True

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        kid = c.child[self._field_index(schema)]
        if c.validity is None:
            return kid
        return ops.backend_for(c).and_parent_validity(kid, c)

    def output_name(self) -> str:
        return f"{self.child}.{self.name}"

    def __str__(self):
        return self.output_name()


def named_struct(**fields) -> CreateNamedStruct:
    return CreateNamedStruct(list(fields), list(fields.values()))


def get_field(struct_expr, name: str) -> GetStructField:
    return GetStructField(struct_expr, name)


class CreateMap(Expression):
    """create_map(k1, v1, k2, v2, ...) -> MAP column (reference:
    GpuCreateMap). Entries keep source order; lookups are last-win."""

    def __init__(self, exprs):
        assert exprs and len(exprs) % 2 == 0, \
            "create_map needs key1, value1, key2, value2, ..."
        self.keys = [_as_expr(e) for e in exprs[0::2]]
        self.vals = [_as_expr(e) for e in exprs[1::2]]

    @property
    def children(self):
        return tuple(self.keys) + tuple(self.vals)

    def dtype(self, schema: Schema) -> DType:
        return DType.map_(self.keys[0].dtype(schema),
                          self.vals[0].dtype(schema))

    def nullable(self, schema: Schema) -> bool:
        return False

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        kc = [e.eval(batch, schema) for e in self.keys]
        vc = [e.eval(batch, schema) for e in self.vals]
        return ops.make_map(kc, vc)

    def output_name(self) -> str:
        return "map"

    def __str__(self):
        inner = ", ".join(f"{k}, {v}" for k, v in zip(self.keys, self.vals))
        return f"map({inner})"


class MapView(Expression):
    """map_keys / map_values / map_entries (zero-copy layout views;
    reference: GpuMapKeys/GpuMapValues/GpuMapEntries)."""

    def __init__(self, child, mode: str):
        self.child = _as_expr(child)
        self.mode = mode  # keys | values | entries

    @property
    def children(self):
        return (self.child,)

    def dtype(self, schema: Schema) -> DType:
        mt = self.child.dtype(schema)
        if mt.id is not TypeId.MAP:
            raise TypeError(f"map_{self.mode} on non-map {mt}")
        if self.mode == "keys":
            return DType.list_(mt.children[0])
        if self.mode == "values":
            return DType.list_(mt.children[1])
        return DType.list_(mt.entry_dtype)

    def eval(self, batch: ColumnBatch, schema: Schema) -> Column:
        c = self.child.eval(batch, schema)
        fn = {"keys": ops.map_keys, "values": ops.map_values,
              "entries": ops.map_entries}[self.mode]
        return fn(c)

    def output_name(self) -> str:
        return f"map_{self.mode}({self.child.output_name()})"

    def __str__(self):
        return f"map_{self.mode}({self.child})"


def create_map(*exprs) -> CreateMap:
    return CreateMap(list(exprs))


def map_keys(m) -> MapView:
    return MapView(m, "keys")


def map_values(m) -> MapView:
    return MapView(m, "values")


def map_entries(m) -> MapView:
    return MapView(m, "entries")
