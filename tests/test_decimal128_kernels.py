"""Decimal kernels (native/hipdf/kernels/decimal128.hip) against exact
integer arithmetic at word, precision and rounding boundaries.

The expected value of every row comes from tests/decimal_ref.py (Python
ints only). Each GPU test drives the kernels through the gpu_backend entry
points, and also checks that cpu_backend agrees with the same oracle.

The oracle's own tests at the top need no GPU and carry no mark, which is
why the `gpu` mark sits on each kernel test and not on the module.
"""
import decimal
import functools
import itertools
import math
import random
from decimal import Decimal
from fractions import Fraction

import pytest

from spark_rapids_amd import Column, ColumnBatch, DType
from spark_rapids_amd.column import dec128_unpack
from spark_rapids_amd.types import TypeId

from . import decimal_ref as ref

gpu = pytest.mark.gpu

P38 = 10 ** 38
I64_MAX = 2 ** 63 - 1
I64_MIN = -2 ** 63
SIZES = (1, 63, 64, 65, 129, 1000)  # partial and exact 64-row validity words
D38 = DType.decimal(38, 0)


# ---------------------------------------------------------------------------
# the oracle pinned against decimal.Decimal (no GPU)
# ---------------------------------------------------------------------------

CTX = decimal.Context(prec=120, rounding=decimal.ROUND_HALF_UP)


def _quantize(value: Decimal, scale: int) -> int:
    q = value.quantize(Decimal(1).scaleb(-scale, CTX), context=CTX)
    return int(q.scaleb(scale, CTX))


def test_ref_half_up_div():
    assert ref.half_up_div(5, 2) == 3
    assert ref.half_up_div(-5, 2) == -3
    assert ref.half_up_div(5, -2) == -3
    assert ref.half_up_div(-5, -2) == 3
    assert ref.half_up_div(49, 10) == 5
    assert ref.half_up_div(-49, 100) == 0
    assert ref.half_up_div(-149, 100) == -1
    assert ref.half_up_div(-150, 100) == -2
    assert ref.half_up_div(0, 7) == 0
    for num, den in [(10 ** 40 + 5, 10), (-(10 ** 40) - 5, 10),
                     (2 ** 127 - 1, 3), (-(2 ** 127), 2 ** 64 + 1),
                     (7, 10 ** 30), (5 * 10 ** 29, 10 ** 30)]:
        want = int(CTX.divide(Decimal(num), Decimal(den)).to_integral_value(
            rounding=decimal.ROUND_HALF_UP, context=CTX))
        assert ref.half_up_div(num, den) == want, (num, den)
    with pytest.raises(ZeroDivisionError):
        ref.half_up_div(1, 0)


def test_ref_mul_div_match_decimal():
    cases = [  # x, y, s1, s2, out_scale, out_prec
        (125, 200, 2, 2, 4, 15),
        (-310, 7, 2, 2, 4, 15),
        (999999999999999999, -999999999999999999, 9, 9, 2, 38),
        (10 ** 37 + 5, 3, 18, 18, 6, 38),
        (-(10 ** 18 - 1), 10 ** 18 - 1, 0, 18, 6, 38),
        (15, 10, 0, 0, 0, 38), (-15, 10, 1, 0, 0, 38),
    ]
    for x, y, s1, s2, so, po in cases:
        dx = Decimal(x).scaleb(-s1, CTX)
        dy = Decimal(y).scaleb(-s2, CTX)
        m = _quantize(CTX.multiply(dx, dy), so)
        assert ref.mul_ref(x, y, s1, s2, so, po) == \
            (m if abs(m) < 10 ** po else None)
        d = _quantize(CTX.divide(dx, dy), so)
        assert ref.div_ref(x, y, s1, s2, so, po) == \
            (d if abs(d) < 10 ** po else None)
    # hand-checked
    assert ref.mul_ref(125, 200, 2, 2, 4, 15) == 25000        # 1.25 * 2.00
    assert ref.mul_ref(-310, 7, 2, 2, 3, 15) == -217          # -0.217
    assert ref.mul_ref(-310, 7, 2, 2, 2, 15) == -22           # -> -0.22
    assert ref.mul_ref(-310, 75, 2, 2, 2, 15) == -233         # -2.325
    assert ref.div_ref(100, 300, 2, 2, 10, 17) == 3333333333  # 1/3
    assert ref.div_ref(500, 200, 2, 2, 0, 17) == 3            # 2.5 -> 3
    assert ref.div_ref(-500, 200, 2, 2, 0, 17) == -3
    assert ref.div_ref(1, 0, 0, 0, 6, 38) is None
    assert ref.div_ref(None, 3, 0, 0, 6, 38) is None
    assert ref.mul_ref(10 ** 19, 10 ** 19, 0, 0, 0, 38) is None
    assert ref.mul_ref(10 ** 38 - 1, 1, 0, 0, 0, 38) == 10 ** 38 - 1
    # the two overflow rows the kernels used to return as 0
    assert ref.div_ref(10 ** 18 - 2, 3, 0, 18, 6, 38) is None
    assert ref.mul_ref(6135925966969082446936281494819,
                       55457378194056862859874864916869166131,
                       18, 18, 6, 38) is None


def test_ref_rescale_and_compare():
    assert ref.rescale_ref(99995, -1, 4, True) is None   # 99.995 -> 100.00
    assert ref.rescale_ref(99994, -1, 4, True) == 9999
    assert ref.rescale_ref(-99995, -1, 4, True) is None
    assert ref.rescale_ref(225, -1, 9, True) == 23
    assert ref.rescale_ref(-225, -1, 9, True) == -23
    assert ref.rescale_ref(249, -2, 9, True) == 2
    assert ref.rescale_ref(-249, -2, 9, True) == -2
    assert ref.rescale_ref(7, 37, 38, False) == 7 * 10 ** 37
    assert ref.rescale_ref(10, 37, 38, False) is None
    assert ref.rescale_ref(I64_MAX, 0, 38, False) == I64_MAX
    assert ref.rescale_ref(I64_MAX + 1, 0, 38, True) is None
    assert ref.rescale_ref(None, 3, 38, False) is None
    for v, shift in [(123455, -1), (-123455, -1), (123449, -2),
                     (5 * 10 ** 37, -38), (-(5 * 10 ** 37) + 1, -38)]:
        want = _quantize(Decimal(v).scaleb(shift, CTX), 0)
        assert ref.rescale_ref(v, shift, 38, False) == want
    assert ref.ARITH["add"](2 ** 64 - 1, 1) == 2 ** 64
    assert ref.ARITH["sub"](0, 1) == -1
    assert ref.ARITH["min"](-1, 1) == -1 and ref.ARITH["max"](-1, 1) == 1
    assert ref.ARITH["add"](None, 1) is None
    assert ref.COMPARE["lt"](-(2 ** 126), 2 ** 126) is True
    assert ref.COMPARE["ge"](3, 3) is True and ref.COMPARE["ne"](3, 3) is False
    assert ref.COMPARE["eq"](3, None) is None
    assert ref.wrap_i128(2 ** 127) == -2 ** 127
    assert ref.wrap_i128(-2 ** 127 - 1) == 2 ** 127 - 1


def test_ref_grouped_sum():
    keys = [1, 2, 1, 3, 2, 3]
    vals = [2 ** 100, None, -2 ** 100 - 1, None, 5, None]
    assert ref.grouped_sum(keys, vals) == {1: (-1, 2), 2: (5, 1),
                                           3: (None, 0)}
    assert ref.grouped_sum(keys, vals, sel=[4, 0, 3]) == {
        2: (5, 1), 1: (2 ** 100, 1), 3: (None, 0)}


# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------

def _backends():
    from spark_rapids_amd.ops import cpu_backend, gpu_backend

    return gpu_backend, cpu_backend


def _unscaled(col: Column) -> list:
    """Rows of a host or device column as unscaled ints (bools for BOOL,
    floats for FLOAT64), None where NULL."""
    col = col.cpu()
    valid = col.valid_array()
    if col.dtype.id is TypeId.DECIMAL128:
        vals = dec128_unpack(col.data.numpy()[: 2 * col.size])
    else:
        vals = col.data.numpy()[: col.size].tolist()
        if col.dtype.id is TypeId.BOOL:
            vals = [bool(v) for v in vals]
    assert len(vals) == col.size == len(valid)
    return [v if ok else None for v, ok in zip(vals, valid)]


def _assert_rows(got: list, want: list, what: str, inputs=None):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [(i, got[i], want[i]) + ((inputs[i],) if inputs else ())
           for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} of {len(want)} rows differ, " \
                    f"first (row, got, want, inputs): {bad[:4]}"


def _check_elementwise(call, host_cols, want, what):
    """call(backend, columns) on the GPU and on the CPU backend over the
    same host columns; both results against the oracle's rows."""
    gb, cb = _backends()
    inputs = list(zip(*[_unscaled(c) for c in host_cols]))
    got = _unscaled(call(gb, [c.cuda() for c in host_cols]))
    _assert_rows(got, want, f"gpu {what}", inputs)
    got = _unscaled(call(cb, host_cols))
    _assert_rows(got, want, f"cpu {what}", inputs)


def _log_uniform(rng: random.Random, count: int, max_abs: int,
                 min_value=None) -> list:
    """Signed values whose bit length is uniform in [0, bits(max_abs)], so
    every limb pattern from an empty word to a full one occurs."""
    top = max_abs.bit_length()
    out = []
    for _ in range(count):
        bits = rng.randint(0, top)
        v = (rng.getrandbits(bits) | (1 << (bits - 1))) if bits else 0
        v = min(v, max_abs)
        out.append(-v if rng.random() < 0.5 else v)
    if min_value is not None:
        out = [max(v, min_value) for v in out]
    return out


def _with_nulls(rng: random.Random, values: list, frac=0.1) -> list:
    return [None if rng.random() < frac else v for v in values]


def _signed(values) -> list:
    return sorted({s * v for v in values for s in (1, -1)})


# named 128-bit edge values, all below 10^38 in magnitude
EDGES128 = _signed([
    0, 1, 2, 5, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 2 ** 64,
    2 ** 64 + 1, 2 ** 65 - 1, (5 << 64) | (1 << 63),
    (5 << 64) | ((1 << 63) - 1), (5 << 64), (6 << 64) - 1, 2 ** 126,
    2 ** 126 - 1, 10 ** 19, 10 ** 37, P38 - 1, P38 // 2,
])
# named 64-bit edge values (raw int64 words of a decimal64 column)
EDGES64 = _signed([0, 1, 2, 5, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 10 ** 17,
                   10 ** 18 - 1, 10 ** 18, I64_MAX]) + [I64_MIN]


def _pool128(seed: int, count=300) -> list:
    rng = random.Random(seed)
    vals = EDGES128 + _log_uniform(rng, count, P38 - 1)
    rng.shuffle(vals)
    return vals


def _pool64(seed: int, prec: int, count=300) -> list:
    """Values of a decimal(prec) column: edges and log-uniform magnitudes
    below 10^prec."""
    rng = random.Random(seed)
    top = 10 ** prec - 1
    vals = _signed([0, 1, 2, 3, 5, 7, top, top - 1, top // 2, top // 3])
    vals += _log_uniform(rng, count, top)
    rng.shuffle(vals)
    return vals


def _pool(seed: int, dt: DType, count=300) -> list:
    if dt.id is TypeId.DECIMAL128:
        return _pool128(seed, count)
    return _pool64(seed, dt.precision, count)


def _pairs(seed: int, xs: list, ys: list, extra=()) -> list:
    """Row pairs: the extra named pairs, then the two pools zipped."""
    n = max(len(xs), len(ys))
    rows = list(extra) + [(xs[i % len(xs)], ys[i % len(ys)])
                          for i in range(n)]
    random.Random(seed).shuffle(rows)
    return rows


# ---------------------------------------------------------------------------
# add / sub / min / max and the six compares (k_i128_arith, k_i128_cmp)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _binary_rows() -> tuple:
    """Every ordered pair of named edges (carries and borrows across bit 64,
    low words that differ only in bit 63 under equal high words, +-(10^38-1),
    +-2^126, 0, -1 against +1), then seeded random pairs."""
    rng = random.Random(101)
    rows = list(itertools.product(EDGES128, EDGES128))
    rows += [(2 ** 64 - 1, 1), (0, 1), (2 ** 64, 1), (-(2 ** 64), -1),
             (-1, 1), (1, -1)]
    rows += list(zip(_log_uniform(rng, 400, P38 - 1),
                     _log_uniform(rng, 400, P38 - 1)))
    rng.shuffle(rows)
    return tuple(rows)


def _in_range_for(op: str, x: int, y: int) -> tuple:
    """For add/sub flip y's sign where the exact result would leave 38
    digits: the result then is a difference of same-signed values."""
    if abs(ref.ARITH[op](x, y)) >= P38:
        y = -y
    assert abs(ref.ARITH[op](x, y)) < P38
    return x, y


def _run_binary(rows, null_mode: str, seed: int):
    rng = random.Random(seed)
    for op in list(ref.ARITH) + list(ref.COMPARE):
        pairs = [_in_range_for(op, x, y) for x, y in rows] \
            if op in ("add", "sub") else list(rows)
        xs = [p[0] for p in pairs]
        ys = [p[1] for p in pairs]
        if null_mode in ("both", "lhs"):
            xs = _with_nulls(rng, xs)
        if null_mode == "both":
            ys = _with_nulls(rng, ys)
        fn = ref.ARITH.get(op) or ref.COMPARE[op]
        want = [fn(x, y) for x, y in zip(xs, ys)]
        out = D38 if op in ref.ARITH else DType.bool_()
        cols = [Column.from_pylist(xs, D38), Column.from_pylist(ys, D38)]
        if null_mode == "none":
            assert cols[0].validity is None and cols[1].validity is None
        if null_mode == "lhs" and len(xs) > 60:
            assert cols[0].validity is not None and cols[1].validity is None
        _check_elementwise(
            lambda be, c, op=op, out=out: be.binary_op(op, c[0], c[1], out),
            cols, want, f"{op} n={len(xs)} nulls={null_mode}")


@gpu
@pytest.mark.parametrize("null_mode", ["both", "lhs", "none"])
@pytest.mark.parametrize("n", SIZES)
def test_i128_binary_ops(n, null_mode):
    _run_binary(_binary_rows()[:n], null_mode, seed=n)


@gpu
def test_i128_binary_all_edge_pairs():
    """Every ordered pair of named edges and every random pair."""
    _run_binary(_binary_rows(), "both", seed=5)


@gpu
def test_i128_binary_named_edges():
    """The named pairs alone, unshuffled and without nulls, so a failure
    names the pair."""
    rows = [(2 ** 64 - 1, 1), (0, 1), (-1, 1), (1, -1),
            (2 ** 64, -1), (-(2 ** 64), 1), (2 ** 64 - 1, 2 ** 64 - 1),
            ((5 << 64) | (1 << 63), (5 << 64) | ((1 << 63) - 1)),
            ((-5 << 64) | (1 << 63), (-5 << 64) | ((1 << 63) - 1)),
            (P38 - 1, -(P38 - 1)), (-(P38 - 1), P38 - 1),
            (P38 - 1, P38 - 1), (2 ** 126, -(2 ** 126)),
            (2 ** 126, 2 ** 126 - 1), (0, 0), (-(2 ** 126), 2 ** 126)]
    _run_binary(rows, "none", seed=0)


@gpu
def test_i128_add_sub_beyond_38_digits():
    """k_i128_arith has no precision check: a sum past 10^38 is not nulled.
    Both backends return the exact sum wrapped to 128 bits, valid: 10^38
    itself where it still fits the words, a sign flip once it passes
    2^127. (Spark nulls such rows in the cast that follows the add.)"""
    gb, cb = _backends()
    xs = [P38 - 1, P38 - 1, -(P38 - 1), 2 ** 126, -(2 ** 126), P38 - 1]
    ys = [1, P38 - 1, -(P38 - 1), 2 ** 126, -(2 ** 126) - 1, -(P38 - 1)]
    for op, flip in (("add", 1), ("sub", -1)):
        yy = [flip * y for y in ys]
        exact = [ref.ARITH[op](x, y) for x, y in zip(xs, yy)]
        assert any(abs(e) >= P38 for e in exact)
        assert any(e != ref.wrap_i128(e) for e in exact)
        want = [ref.wrap_i128(e) for e in exact]
        cols = [Column.from_pylist(xs, D38), Column.from_pylist(yy, D38)]
        g = _unscaled(gb.binary_op(op, cols[0].cuda(), cols[1].cuda(), D38))
        c = _unscaled(cb.binary_op(op, cols[0], cols[1], D38))
        assert g == c, (op, g, c)
        assert g == want, (op, g, want)


# ---------------------------------------------------------------------------
# k_i128_rescale / k_i64_to_i128 through decimal -> decimal cast
# ---------------------------------------------------------------------------

def _fits_storage(v: int, dt: DType) -> bool:
    if dt.id is TypeId.DECIMAL128:
        return -2 ** 127 <= v < 2 ** 127
    return I64_MIN <= v <= I64_MAX


def _rescale_values(seed: int, src: DType, to: DType) -> list:
    """Source pool plus, for this (shift, precision): ties on both signs,
    the values that land on 10^p - 1 and on 10^p, and the int64 limits."""
    rng = random.Random(seed)
    shift = to.scale - src.scale
    bound = 10 ** to.precision
    if src.id is TypeId.DECIMAL128:
        vals = EDGES128 + _log_uniform(rng, 300, P38 - 1)
    else:
        vals = EDGES64 + _log_uniform(rng, 300, I64_MAX, I64_MIN)
    named = [I64_MAX, I64_MAX + 1, 10 ** 18 - 1, 10 ** 18]
    if shift < 0:
        k = -shift
        half = 5 * 10 ** (k - 1)
        for m in (0, 1, 12345, 10 ** 10 + 1):
            named += [m * 10 ** k + half, m * 10 ** k + half - 1]
        named += [bound * 10 ** k - half, bound * 10 ** k - half - 1,
                  I64_MAX * 10 ** k + half - 1, I64_MAX * 10 ** k + half]
    else:
        if to.precision >= shift:
            named += [10 ** (to.precision - shift),
                      10 ** (to.precision - shift) - 1]
        named += [2 ** 128 // 10 ** shift, 2 ** 128 // 10 ** shift + 1,
                  10 ** 37, 3 * 10 ** 37]
    vals += [v for v in _signed(named) if _fits_storage(v, src)]
    rng.shuffle(vals)
    return vals


def _check_rescale(vals: list, src: DType, to: DType, what=""):
    shift = to.scale - src.scale
    want = [ref.rescale_ref(v, shift, to.precision,
                            to.id is TypeId.DECIMAL64) for v in vals]
    _check_elementwise(lambda be, c: be.cast(c[0], to),
                       [Column.from_pylist(vals, src)], want,
                       f"cast {src} -> {to} {what}")
    return want


# (source, target, can overflow). A down-shift or a plain widening into 38
# digits cannot overflow, and neither can an int64 times 10^19 (< 10^38).
RESCALE_CASES = [
    ((38, 38), (38, 0), False),  # shift -38
    ((38, 19), (38, 0), False),  # -19
    ((38, 18), (38, 0), False),  # -18
    ((38, 1), (38, 0), False),   # -1
    ((38, 0), (38, 1), True),    # +1
    ((38, 0), (38, 18), True),   # +18
    ((38, 0), (38, 19), True),   # +19
    ((38, 0), (38, 37), True),   # +37: most products overflow u128
    ((38, 2), (20, 2), True),    # shift 0, 20 digits: 10^20 - 1 and 10^20
    ((38, 3), (20, 2), True),    # rounding carries into 10^20
    ((38, 0), (18, 0), True),    # narrowing to decimal64
    ((38, 4), (18, 2), True),    # narrowing with a down-shift
    ((38, 0), (18, 18), True),   # narrowing with an up-shift
    ((5, 3), (4, 2), True),      # decimal64 -> decimal64: 99.995 -> NULL
    ((18, 6), (9, 2), True),
    ((18, 0), (38, 0), False),   # k_i64_to_i128 widening, int64 min and max
    ((18, 0), (38, 19), False),  # widening, then a product past int64
    ((18, 18), (38, 0), False),  # widening, then -18
]


@gpu
@pytest.mark.parametrize("case", RESCALE_CASES, ids=lambda c: f"{c[0]}to{c[1]}")
def test_rescale_cases(case):
    src, to = DType.decimal(*case[0]), DType.decimal(*case[1])
    rng = random.Random(7)
    vals = _with_nulls(rng, _rescale_values(11, src, to))
    want = _check_rescale(vals, src, to)
    # the case must reach the outcomes it is there for
    assert any(w is None and v is not None
               for v, w in zip(vals, want)) == case[2]
    assert any(w is not None for w in want)


@gpu
@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_rescale_sizes(n, nulls):
    rng = random.Random(n)
    for s, t in (((38, 18), (38, 0)), ((38, 0), (18, 0)), ((18, 0), (38, 3))):
        src, to = DType.decimal(*s), DType.decimal(*t)
        vals = _rescale_values(13, src, to)
        vals = (vals * (n // len(vals) + 1))[:n]
        if nulls:
            vals = _with_nulls(rng, vals)
        col = Column.from_pylist(vals, src)
        assert nulls or col.validity is None
        _check_rescale(vals, src, to, f"n={n}")


@gpu
def test_rescale_hand_checked():
    """Literal expectations, each also equal to the oracle's."""
    def run(vals, s, t):
        return _check_rescale(vals, DType.decimal(*s), DType.decimal(*t))

    # ties go away from zero, ...49 goes toward zero, on both signs
    assert run([225, -225, 249, -249, 5, -5, 4, -4], (9, 2), (9, 1)) == \
        [23, -23, 25, -25, 1, -1, 0, 0]
    assert run([249, -249, 250, -250, 49, -49, 50, -50], (9, 2), (9, 0)) == \
        [2, -2, 3, -3, 0, 0, 1, -1]
    assert run([12345 * 10 ** 19 + 5 * 10 ** 18,
                -(12345 * 10 ** 19 + 5 * 10 ** 18),
                12345 * 10 ** 19 + 5 * 10 ** 18 - 1,
                -(12345 * 10 ** 19 + 5 * 10 ** 18 - 1)],
               (38, 19), (38, 0)) == [12346, -12346, 12345, -12345]
    # 99.995 at decimal(5,3) rounds to 100.00: one digit too many
    assert run([99995, -99995, 99994, -99994], (5, 3), (4, 2)) == \
        [None, None, 9999, -9999]
    # exactly 10^p - 1 and 10^p
    assert run([10 ** 20 - 1, 10 ** 20, -(10 ** 20 - 1), -(10 ** 20)],
               (38, 2), (20, 2)) == [10 ** 20 - 1, None, -(10 ** 20 - 1), None]
    # narrowing to decimal64
    assert run([10 ** 18 - 1, 10 ** 18, I64_MAX, -I64_MAX, -(10 ** 18 - 1)],
               (38, 0), (18, 0)) == \
        [10 ** 18 - 1, None, None, None, -(10 ** 18 - 1)]
    # an up-shift whose product overflows u128, and one that only passes
    # 10^38
    assert run([10 ** 37, 4 * 10 ** 37, 9, 10, -10], (38, 0), (38, 37)) == \
        [None, None, 9 * 10 ** 37, None, None]
    # sign extension of the int64 limits
    assert run([I64_MIN, I64_MAX, -1, 0], (18, 0), (38, 0)) == \
        [I64_MIN, I64_MAX, -1, 0]
    assert run([I64_MIN, I64_MAX], (18, 0), (38, 19)) == \
        [I64_MIN * 10 ** 19, I64_MAX * 10 ** 19]


# ---------------------------------------------------------------------------
# multiply / divide (k_dec64_mul_div, k_dec_mul_div_wide)
# ---------------------------------------------------------------------------

def _op_shift(op, a: DType, b: DType, out: DType) -> int:
    return a.scale + b.scale - out.scale if op == "mul" \
        else out.scale + b.scale - a.scale


def _tie_pairs(op, a: DType, b: DType, out: DType) -> list:
    """Operand pairs whose exact result ends in .5 at the output scale (and
    their neighbours), on every sign combination, where they fit."""
    shift = _op_shift(op, a, b, out)
    odd = [1, 3, 12345, 10 ** 9 + 7]
    pairs = []
    if op == "mul":
        if shift > 0:  # x*y = odd * 10^shift / 2
            pairs = [(x, 5 * 10 ** (shift - 1)) for x in odd]
            pairs += [(5 * 10 ** (shift - 1), x) for x in odd]
    elif shift >= 0:   # x * 10^shift / 2^(shift+1) = x * 5^shift / 2
        pairs = [(x, 2 ** (shift + 1)) for x in odd]
    else:              # x / (y * 10^k) with x = odd * y * 10^k / 2
        k = -shift
        pairs = [(x * y * 5 * 10 ** (k - 1), y) for x in odd for y in (1, 3)]
    pairs += [(x + 1, y) for x, y in pairs] + [(x - 1, y) for x, y in pairs]
    pairs = [(sx * x, sy * y) for x, y in pairs
             for sx in (1, -1) for sy in (1, -1)]
    return [(x, y) for x, y in pairs
            if abs(x) < 10 ** a.precision and abs(y) < 10 ** b.precision]


def _check_mul_div(op, a: DType, b: DType, out: DType, rows,
                   null_mode="none", seed=3) -> list:
    """decimal_mul_div over the row pairs on both backends against the
    oracle; returns the oracle's rows."""
    assert len(rows) <= 1000  # the wide division loops digit by digit
    rng = random.Random(seed)
    xs = [r[0] for r in rows]
    ys = [r[1] for r in rows]
    if null_mode in ("both", "lhs"):
        xs = _with_nulls(rng, xs)
    if null_mode == "both":
        ys = _with_nulls(rng, ys)
    fn = ref.mul_ref if op == "mul" else ref.div_ref
    want = [fn(x, y, a.scale, b.scale, out.scale, out.precision)
            for x, y in zip(xs, ys)]
    if out.id is TypeId.DECIMAL64:
        assert all(w is None or abs(w) <= I64_MAX for w in want)
    cols = [Column.from_pylist(xs, a), Column.from_pylist(ys, b)]
    if null_mode == "none":
        assert cols[0].validity is None and cols[1].validity is None
    _check_elementwise(
        lambda be, c: be.decimal_mul_div(op, c[0], c[1], out), cols, want,
        f"{op} {a} {b} -> {out} n={len(xs)} nulls={null_mode}")
    return want, xs, ys


def _check_rows(op, a, b, out, rows) -> list:
    return _check_mul_div(op, a, b, out, rows)[0]


def _check_table_case(op, a, b, out, rows, overflows: bool):
    """A table case with nulls on both sides; it must reach an overflow NULL
    exactly where its types allow one, and a valid row always."""
    want, xs, ys = _check_mul_div(op, a, b, out, rows, "both")
    over = any(w is None and x is not None and y not in (None, 0)
               for x, y, w in zip(xs, ys, want))
    assert over == overflows, "overflow rows"
    assert any(w is not None for w in want), "no valid row"


def _table_rows(op, a: DType, b: DType, out: DType, extra=()) -> list:
    named = []
    if a.id is TypeId.DECIMAL64 and b.id is TypeId.DECIMAL64:
        named = list(itertools.product(_pool(0, a, 0), _pool(0, b, 0)))
    named += _tie_pairs(op, a, b, out) + list(extra)
    if op == "div":
        named += [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -7)]
    return _pairs(5, _pool(21, a), _pool(22, b), named)


def _dt(spec) -> DType:
    return DType.decimal(*spec)


# Each case is (lhs, rhs, out, can overflow): whether the largest operands
# of these types give more digits than `out` holds. A zero divisor is not
# counted as an overflow.
DEC64_MUL = [
    ((9, 2), (8, 4), (18, 6), False),      # decimal64 out, shift 0
    ((18, 9), (18, 9), (18, 2), True),     # decimal64 out, shift 16
    ((18, 2), (18, 4), (38, 6), False),    # decimal128 out, shift 0
    ((18, 2), (18, 4), (38, 2), False),    # shift 4
    ((18, 0), (18, 0), (35, 0), True),     # 36-digit products, 35 kept
    ((18, 18), (18, 18), (38, 6), False),  # shift 30
]
# the shift is out.scale + rhs.scale - lhs.scale
DEC64_DIV = [
    ((18, 10), (18, 0), (38, 4), False),   # -6
    ((18, 10), (18, 0), (18, 4), False),   # -6, decimal64 out
    ((18, 6), (18, 0), (38, 6), False),    # 0
    ((18, 6), (18, 0), (17, 6), True),     # 0, quotients at 17 digits
    ((18, 2), (18, 4), (38, 6), False),    # 8
    ((7, 2), (7, 2), (17, 10), False),     # 10, decimal64 out
    ((18, 0), (18, 12), (38, 6), False),   # 18, one full chunk
]
# shifts 19..36 take a second chunk; from 21 on small divisors overflow the
# partial quotient there
DEC64_DIV_LONG = [
    ((18, 0), (18, 13), (38, 6), False),   # 19
    ((18, 0), (18, 18), (38, 6), True),    # 24
    ((18, 0), (18, 18), (38, 18), True),   # 36
]


def _ids(c):
    return "-".join(f"{p}.{s}" for p, s in c[:3])


@gpu
@pytest.mark.parametrize("case", DEC64_MUL, ids=_ids)
def test_dec64_mul_table(case):
    a, b, out = map(_dt, case[:3])
    _check_table_case("mul", a, b, out, _table_rows("mul", a, b, out),
                      case[3])


@gpu
@pytest.mark.parametrize("case", DEC64_DIV, ids=_ids)
def test_dec64_div_table(case):
    a, b, out = map(_dt, case[:3])
    _check_table_case("div", a, b, out, _table_rows("div", a, b, out),
                      case[3])


def _resized(rows: list, n: int) -> list:
    return (rows * (n // len(rows) + 1))[:n]


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_dec64_mul_div_sizes(n):
    a, b = _dt((18, 2)), _dt((18, 4))
    rows = _resized(_table_rows("div", a, b, _dt((38, 6))), n)
    for mode in ("both", "lhs", "none"):
        for op, out in (("mul", (38, 2)), ("mul", (18, 6)), ("div", (38, 6))):
            _check_mul_div(op, a, b, _dt(out), rows, mode, seed=n)


@gpu
@pytest.mark.parametrize("case", ["pair", "sample"] + DEC64_DIV_LONG,
                         ids=lambda c: c if isinstance(c, str) else _ids(c))
def test_dec64_div_overflow_is_null(case):
    """A partial quotient that no longer fits 128 bits means the result has
    more than 38 digits: NULL. The kernel used to mark such a row with an
    all-ones quotient and then round it, which wrapped it to a valid 0."""
    if isinstance(case, str):
        a, b, out = _dt((18, 0)), _dt((18, 18)), _dt((38, 6))
        if case == "pair":
            assert _check_rows("div", a, b, out, [(10 ** 18 - 2, 3)]) == [None]
            return
        rng = random.Random(20000)
        rows = [(rng.randint(-(10 ** 18 - 1), 10 ** 18 - 1),
                 rng.randint(-999, 999)) for _ in range(2000)]
        for lo in (0, 1000):
            want = _check_rows("div", a, b, out, rows[lo:lo + 1000])
            # x * 10^24 / y has 39 digits or more once |x| > |y| * 10^14
            assert sum(w is None for w in want) > 900
        return
    a, b, out = map(_dt, case[:3])
    _check_table_case("div", a, b, out, _table_rows("div", a, b, out),
                      case[3])


NEAR38 = _signed([P38 - 1, P38 - 2, P38 // 3, 7 * 10 ** 37 + 11,
                  35 * 10 ** 36 + 1, 5 * 10 ** 37 + 3, 2 ** 126, 10 ** 37])
WIDE_MUL = [  # lhs, rhs, out, can overflow
    ((38, 0), (38, 0), (38, 0), True),     # shift 0
    ((38, 1), (38, 0), (38, 0), True),     # 1
    ((38, 3), (38, 3), (38, 0), True),     # 6
    ((38, 18), (38, 18), (38, 6), True),   # 30
    # 38: four-limb products that fit again, (10^38-1)^2 / 10^38 < 10^38
    ((38, 20), (38, 18), (38, 0), False),
    ((18, 4), (38, 10), (38, 6), True),    # 64 x 128
    ((38, 10), (18, 4), (38, 6), True),    # 128 x 64
    ((38, 10), (18, 4), (18, 2), True),    # decimal64 out
]
WIDE_DIV = [
    ((38, 6), (38, 6), (38, 0), False),    # shift 0
    ((38, 0), (38, 0), (38, 6), True),     # 6
    ((38, 0), (38, 0), (38, 30), True),    # 30
    ((38, 0), (38, 18), (38, 19), True),   # 37
    ((38, 0), (38, 0), (20, 0), True),     # 0, quotients at 20 digits
    ((38, 10), (38, 0), (38, 4), False),   # -6
    ((38, 30), (38, 0), (38, 0), False),   # -30: y * 10^30 passes 2^128
    ((18, 2), (38, 10), (38, 6), False),   # 64 / 128
    ((38, 10), (18, 2), (38, 6), False),   # 128 / 64
    ((38, 10), (18, 2), (18, 4), True),    # decimal64 out
]


def _wide_rows(op, a, b, out) -> list:
    extra = []
    if a.id is TypeId.DECIMAL128 and b.id is TypeId.DECIMAL128:
        # both operands near 10^38: four-limb products, and divisors above
        # 3.5e37 whose remainder times ten needs the 192-bit path
        extra += list(itertools.product(NEAR38, NEAR38))
        extra += [(y + d, y) for y in NEAR38 for d in (-1, 0, 1)
                  if abs(y + d) < P38]
        extra += [(x, s) for x in NEAR38 for s in (1, -1)]  # divisor 1
        extra += [(0, y) for y in NEAR38[:4]]
        # quotients at the 20-digit bound: 10^20 - 0.5 and 10^20 - 1.5
        extra += [(2 * 10 ** 20 - 1, 2), (2 * 10 ** 20 - 3, 2),
                  (-(2 * 10 ** 20 - 1), 2), (10 ** 20, 1), (10 ** 20 - 1, -1)]
        # and at 38 digits for an up-shift of 6
        extra += [(10 ** 32 - 1, 1), (10 ** 32, 1), (-(10 ** 32), 1)]
    return _table_rows(op, a, b, out, extra)


@gpu
@pytest.mark.parametrize("case", WIDE_MUL, ids=_ids)
def test_wide_mul_table(case):
    a, b, out = map(_dt, case[:3])
    _check_table_case("mul", a, b, out, _wide_rows("mul", a, b, out), case[3])


@gpu
@pytest.mark.parametrize("case", WIDE_DIV, ids=_ids)
def test_wide_div_table(case):
    a, b, out = map(_dt, case[:3])
    _check_table_case("div", a, b, out, _wide_rows("div", a, b, out), case[3])


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_wide_mul_div_sizes(n):
    a, b, out = _dt((38, 18)), _dt((38, 18)), _dt((38, 6))
    rows = _resized(_wide_rows("div", a, b, out), n)
    for mode in ("both", "lhs", "none"):
        _check_mul_div("mul", a, b, out, rows, mode, seed=n)
        _check_mul_div("div", a, b, out, rows, mode, seed=n)


@gpu
def test_dec64_operands_both_64_take_dec64_kernel():
    """decimal_mul_div sends two 64-bit operands to k_dec64_mul_div, so of
    the four width combinations the wide kernel sees three; the fourth is
    this one, at types the tables above do not repeat."""
    a, b, out = _dt((18, 6)), _dt((18, 6)), _dt((38, 6))
    _check_table_case("mul", a, b, out, _table_rows("mul", a, b, out), False)
    _check_table_case("div", a, b, out, _table_rows("div", a, b, out), False)


@gpu
def test_wide_mul_round_wrap_is_null():
    """After the 30 digits are removed the two low limbs are all ones and
    the last digit removed is 8: rounding up used to wrap the magnitude to
    a valid 0. The exact product has 39 digits: NULL."""
    a = b = _dt((38, 18))
    x, y = 6135925966969082446936281494819, \
        55457378194056862859874864916869166131
    q, r = divmod(x * y, 10 ** 30)
    assert q == 2 ** 128 - 1 and r * 10 // 10 ** 30 >= 5
    rows = [(sx * x, sy * y) for sx in (1, -1) for sy in (1, -1)]
    rows += [(y, x), (x, 1), (1, y)]
    want = _check_rows("mul", a, b, _dt((38, 6)), rows)
    assert want[:5] == [None] * 5 and want[5] is not None


@gpu
def test_wide_mul_results_at_38_digits():
    """Products that land exactly on 10^38 - 1 (valid) and 10^38 (NULL),
    without rounding and through it."""
    x5, x6 = 58823529411764705882352941176470588235, \
        71428571428571428571428571428571428571
    assert x5 * 17 == 10 ** 39 - 5 and x6 * 14 == 10 ** 39 - 6
    a, b = _dt((38, 1)), _dt((38, 0))
    want = _check_rows(
        "mul", a, b, _dt((38, 0)),
        [(x5, 17), (x6, 14), (-x5, 17), (x6, -14), (17, x5), (14, -x6)])
    assert want == [None, P38 - 1, None, -(P38 - 1), None, -(P38 - 1)]
    a = b = _dt((38, 0))
    want = _check_rows(
        "mul", a, b, _dt((38, 0)),
        [(P38 - 1, 1), (10 ** 19, 10 ** 19), (-(10 ** 19), 10 ** 19),
         (P38 - 1, -1), (P38 - 1, P38 - 1), (10 ** 19 - 1, 10 ** 19 + 1)])
    assert want == [P38 - 1, None, None, -(P38 - 1), None, P38 - 1]


@gpu
def test_wide_div_huge_denominator_rounds_to_zero():
    """A negative shift multiplies the divisor by 10^k. Once y * 10^k passes
    2^128 it is more than twice any 128-bit dividend, so the exact quotient
    rounds to 0: a valid 0.000..., which is what BigDecimal division and the
    CPU backend give. The kernel used to null these rows because the scaled
    divisor did not fit its u128."""
    a, b, out = _dt((38, 30)), _dt((38, 0)), _dt((38, 0))
    rows = [(P38 - 1, 10 ** 9), (-(P38 - 1), 10 ** 9), (P38 - 1, P38 - 1),
            (1, -(P38 - 1)), (0, 10 ** 9), (2 ** 126, 2 ** 128 // 10 ** 30 + 1),
            # the largest divisor that still fits, and small ones
            (P38 - 1, 2 ** 128 // 10 ** 30), (P38 - 1, 7), (5 * 10 ** 29, 1),
            (5 * 10 ** 29 - 1, -1), (3, 0)]
    want = _check_rows("div", a, b, out, rows)
    assert want == [0, 0, 0, 0, 0, 0, 0, 14285714, 1, 0, None]


# ---------------------------------------------------------------------------
# k_i128_to_f64 through cast(decimal128 -> double)
# ---------------------------------------------------------------------------

F64_NAMED = [-1, -5, -1024, -1025, -5000, -1234, 0, 1, 5] + _signed([
    2 ** 53 + 1, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, 2 ** 64 + 2 ** 11 + 1,
    2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 - 1, 2 ** 117 + 2 ** 64 + 1,
    2 ** 117 + 2 ** 64, 2 ** 126 + 2 ** 73, 2 ** 126 + 2 ** 73 + 1,
    2 ** 126 + 2 ** 73 - 1, 2 ** 126 + 3 * 2 ** 73, P38 - 1])


def _f64_values() -> list:
    rng = random.Random(53)
    vals = F64_NAMED + _log_uniform(rng, 400, P38 - 1)
    return vals


def _cast_f64(vals, scale):
    gb, cb = _backends()
    col = Column.from_pylist(vals, DType.decimal(38, scale))
    g = _unscaled(gb.cast(col.cuda(), DType.float64()))
    c = _unscaled(cb.cast(col, DType.float64()))
    return g, c


def _check_sign(got: float, v: int, what):
    assert (got == 0.0) == (v == 0), (what, v, got)
    assert math.copysign(1.0, got) == (1.0 if v >= 0 else -1.0), (what, v, got)


@gpu
@pytest.mark.parametrize("nulls", [False, True])
def test_i128_to_f64_scale0_exact(nulls):
    """At scale 0 the cast is the correctly rounded double of the integer:
    Python's float(v), and BigDecimal.doubleValue in Spark."""
    vals = _f64_values()
    if nulls:
        vals = _with_nulls(random.Random(1), vals)
    want = [None if v is None else float(v) for v in vals]
    g, c = _cast_f64(vals, 0)
    _assert_rows(g, want, "gpu cast decimal(38,0) -> double", vals)
    _assert_rows(c, want, "cpu cast decimal(38,0) -> double", vals)
    for v, x in zip(vals, g):
        if v is not None:
            _check_sign(x, v, "gpu")


@gpu
@pytest.mark.parametrize("scale", [2, 10, 22])
def test_i128_to_f64_scaled_within_one_ulp(scale):
    """With a scale both backends divide the rounded double by 10^scale: two
    correctly rounded steps, each off by at most half an ulp, so the result
    is within 1 ulp of the correctly rounded quotient. The scales stop at
    22, the last power of ten a double holds exactly; past it the divisor
    would add a third rounding that this budget does not cover."""
    assert float(10 ** scale) == 10 ** scale
    vals = _with_nulls(random.Random(scale), _f64_values())
    g, c = _cast_f64(vals, scale)
    assert len(g) == len(c) == len(vals)
    bad = []
    for i, v in enumerate(vals):
        if v is None:
            assert g[i] is None and c[i] is None, i
            continue
        want = float(Fraction(v, 10 ** scale))
        for name, got in (("gpu", g[i]), ("cpu", c[i])):
            assert got is not None, (name, i, v)
            _check_sign(got, v, name)
            if abs(got - want) > math.ulp(want):
                bad.append((name, v, got, want))
    assert not bad, (len(bad), bad[:4])


@gpu
def test_i128_to_f64_issue_example():
    """cast(decimal(30,2) as double) of -12.34 is -12.34."""
    gb, cb = _backends()
    dt = DType.decimal(30, 2)
    vals = [-1234, -5, -5000, 1234, None]
    col = Column.from_pylist(vals, dt)
    want = [-12.34, -0.05, -50.0, 12.34, None]
    assert _unscaled(gb.cast(col.cuda(), DType.float64())) == want
    assert _unscaled(cb.cast(col, DType.float64())) == want


# ---------------------------------------------------------------------------
# grouped sums (k_gb_sum_i128_lds, k_gb_sum_i64_to_i128, k_gb_sum_i128)
# ---------------------------------------------------------------------------

GB_ROWS = 10000


@functools.lru_cache(maxsize=None)
def _gb_inputs(width: int, ngroups: int) -> tuple:
    """(keys, values). Half of the rows fall into the first few groups, so
    that there the low word wraps many times in both directions and the
    running high word goes negative; the last group is entirely NULL."""
    rng = random.Random(1000 * width + ngroups)
    hot = min(ngroups, 4)
    keys = [rng.randrange(hot) if rng.random() < 0.5
            else rng.randrange(ngroups) for _ in range(GB_ROWS)]
    keys[:ngroups] = range(ngroups)  # every group occurs
    if width == 64:
        big = [I64_MAX, -I64_MAX, I64_MIN, I64_MAX - 1, 2 ** 62, -(2 ** 62)]
    else:
        big = _signed([2 ** 64 - 1, 2 ** 100, 2 ** 64, 2 ** 63,
                       2 ** 100 + 2 ** 64 - 1])
    vals = []
    for _ in range(GB_ROWS):
        r = rng.random()
        if r < 0.1:
            vals.append(None)
        elif r < 0.6:
            vals.append(rng.choice(big))
        elif r < 0.8:
            vals.append(rng.randint(-1000, 1000))
        else:
            vals.append(_log_uniform(rng, 1, I64_MAX if width == 64
                                     else 2 ** 100)[0])
    if ngroups > 1:
        vals = [None if k == ngroups - 1 else v for k, v in zip(keys, vals)]
    return tuple(keys), tuple(vals)


def _gb_result(batch_out: ColumnBatch) -> dict:
    keys, sums, cnts = (_unscaled(c) for c in batch_out.columns)
    assert len(set(keys)) == len(keys), "a group came out twice"
    return {k: (s, c) for k, s, c in zip(keys, sums, cnts)}


def _check_grouped(width, ngroups, use_sel, null_key=False):
    import torch

    gb, cb = _backends()
    keys, vals = map(list, _gb_inputs(width, ngroups))
    if null_key:
        keys = [None if k == 5 else k for k in keys]
    vdt = DType.decimal(18, 2) if width == 64 else DType.decimal(30, 2)
    out_dt = DType.decimal(38, 2)
    sel = None
    if use_sel:
        sel = list(range(GB_ROWS))
        random.Random(ngroups).shuffle(sel)
        sel = sel[: GB_ROWS // 3]
    want = ref.grouped_sum(keys, vals, sel)
    assert all(t is None or abs(t) < P38 for t, _ in want.values())
    if ngroups > 1 and not use_sel:
        assert want[ngroups - 1] == (None, 0)
        assert len(want) == ngroups
    if ngroups <= 7:
        # the hot groups really cross the word boundary, both ways
        assert any(t is not None and t < -(2 ** 64) for t, _ in want.values()) \
            or any(t is not None and t > 2 ** 64 for t, _ in want.values())
    aggs = [("sum", 1, out_dt), ("count", 1, DType.int64())]
    batch = ColumnBatch([Column.from_pylist(keys, DType.int32()),
                         Column.from_pylist(vals, vdt)])
    dev_sel = None if sel is None else \
        torch.tensor(sel, dtype=torch.int32).cuda()
    got = _gb_result(gb.group_by_aggregate(batch.cuda(), [0], aggs, dev_sel))
    assert got == want, _gb_diff(got, want)
    if sel is not None:  # the CPU backend takes no sel: gather the rows
        batch = ColumnBatch([
            Column.from_pylist([keys[i] for i in sel], DType.int32()),
            Column.from_pylist([vals[i] for i in sel], vdt)])
    got = _gb_result(cb.group_by_aggregate(batch, [0], aggs))
    assert got == want, _gb_diff(got, want)


def _gb_diff(got: dict, want: dict):
    bad = [(k, got.get(k), want.get(k)) for k in sorted(
        set(got) | set(want), key=lambda k: (k is None, k))
        if got.get(k) != want.get(k)]
    return f"{len(bad)} groups differ, first (key, got, want): {bad[:4]}"


@gpu
@pytest.mark.parametrize("use_sel", [False, True], ids=["all", "sel"])
@pytest.mark.parametrize("ngroups", [1, 7, 2048, 2049, 3000])
@pytest.mark.parametrize("width", [64, 128])
def test_grouped_sum(width, ngroups, use_sel):
    """2048 groups is the last size of the LDS kernel; 2049 and 3000 run
    the per-row atomic kernels, one for each input width."""
    _check_grouped(width, ngroups, use_sel)


@gpu
@pytest.mark.parametrize("ngroups", [7, 2049])
@pytest.mark.parametrize("width", [64, 128])
def test_grouped_sum_nullable_key(width, ngroups):
    """A key column with a validity buffer takes the hash path to the same
    kernels; the NULL key is a group of its own."""
    _check_grouped(width, ngroups, False, null_key=True)
