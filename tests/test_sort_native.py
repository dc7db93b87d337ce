"""The multi-key radix sort as one native call (ext.sort_order) with
device-decided skipping of constant digits.

Oracle: per key, dense integer codes on the CPU in the requested direction
with nulls placed as requested (strings by UTF-8 bytes, floats in Spark
order: NaN greatest, -0.0 == 0.0), then np.lexsort over the codes. lexsort
is stable and so is an LSD radix sort, so the expected permutation is unique
and the GPU permutation is compared for exact equality."""
import numpy as np
import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, ColumnBatch, DType
from spark_rapids_amd.types import (FLOAT32, FLOAT64, INT8, INT16, INT32,
                                    INT64, STRING)

pytestmark = pytest.mark.gpu

D128 = DType.decimal(20, 2)  # 128-bit backed

# 40 000 rows = 10 radix tiles -> 2560 counts -> two scan levels
SIZES = [1, 2, 255, 4095, 4096, 4097, 40_000]


def _key_of(v):
    """Total-order key of one non-null python value."""
    if isinstance(v, str):
        return v.encode("utf-8")
    if isinstance(v, float):
        return (1, 0.0) if v != v else (0, v + 0.0)  # NaN greatest, -0 == 0
    return v


def _codes(vals, desc, nulls_last):
    uniq = sorted({_key_of(v) for v in vals if v is not None})
    rank = {k: i for i, k in enumerate(uniq)}
    top = len(uniq)
    out = np.empty(len(vals), dtype=np.int64)
    for i, v in enumerate(vals):
        if v is None:
            out[i] = top if nulls_last else -1
        else:
            r = rank[_key_of(v)]
            out[i] = top - 1 - r if desc else r
    return out


def _expected(keys, descending, nulls_last):
    """keys: python value lists, most significant first."""
    codes = [_codes(v, d, nl)
             for v, d, nl in zip(keys, descending, nulls_last)]
    return np.lexsort(tuple(reversed(codes))).astype(np.int32)


def _column(vals, dtype):
    """vals: python list with None for null; floats / ints go through numpy
    so their bit patterns (NaN, -0.0, float32) arrive unchanged."""
    if dtype.id.value == "string" or dtype is D128:
        return Column.from_pylist(vals, dtype)
    valid = np.array([v is not None for v in vals], dtype=bool)
    arr = np.array([0 if v is None else v for v in vals],
                   dtype=dtype.numpy_dtype())
    return Column.from_numpy(arr, dtype, None if valid.all() else valid)


def _gpu_perm(cols, descending, nulls_last):
    from spark_rapids_amd.ops import gpu_backend

    batch = ColumnBatch(list(cols)).cuda()
    out = gpu_backend.sort_order(batch, list(range(len(cols))),
                                 list(descending), list(nulls_last))
    assert out.size == cols[0].size and out.validity is None
    return out.cpu().data.numpy()


def _check(keys, dtypes, descending, nulls_last, what=""):
    cols = [_column(v, dt) for v, dt in zip(keys, dtypes)]
    got = _gpu_perm(cols, descending, nulls_last)
    exp = _expected(keys, descending, nulls_last)
    assert np.array_equal(got, exp), \
        f"{what} desc={descending} nulls_last={nulls_last}: first mismatch " \
        f"at {int(np.argmax(got != exp))}"


def _rand_strings(rng, n, maxlen=20):
    alphabet = list("abcXYZ019 _") + ["ö", "√", "\x01"]
    lens = rng.integers(0, maxlen + 1, n)
    return ["".join(rng.choice(alphabet, int(k))) for k in lens]


def _values(name, n, rng):
    """python values (few distinct and many distinct mixed, so ties occur)."""
    if name == "int8":
        return [int(x) for x in rng.integers(-128, 128, n)], INT8
    if name == "int16":
        return [int(x) for x in rng.integers(-2**15, 2**15, n)], INT16
    if name == "int32":
        return [int(x) for x in rng.integers(-2**31, 2**31, n)], INT32
    if name == "int64":
        return [int(x) for x in rng.integers(-2**63, 2**63 - 1, n)], INT64
    if name in ("float32", "float64"):
        dt = FLOAT32 if name == "float32" else FLOAT64
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)) \
            .astype(dt.numpy_dtype())
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5],
                           dtype=dt.numpy_dtype())
        pick = rng.random(n) < 0.1
        a[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        return [float(x) for x in a], dt
    if name == "decimal128":
        hi = rng.integers(-2**20, 2**20, n)
        lo = rng.integers(0, 2**62, n)
        # +-2^66 at most: inside decimal(20,2)'s 10^20, past int64
        return [int(h) * 2**46 + int(l) % 2**46
                for h, l in zip(hi, lo)], D128
    assert name == "string"
    return _rand_strings(rng, n), STRING


def _with_nulls(vals, rng, frac=0.05):
    out = list(vals)
    for i in np.flatnonzero(rng.random(len(out)) < frac):
        out[i] = None
    if len(out) > 1:
        out[0] = None  # position 0 (the diff word's reference row) is null
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["int8", "int16", "int32", "int64",
                                  "float32", "float64", "decimal128",
                                  "string"])
def test_single_key(name, n):
    rng = np.random.default_rng(1000 + n)
    vals, dt = _values(name, n, rng)
    for v in (vals, _with_nulls(vals, rng)):
        for desc in (False, True):
            for nl in (False, True):
                _check([v], [dt], [desc], [nl], f"{name} n={n}")


CONST_N = 5000  # two radix tiles, the second partial


def _const_shapes():
    n = CONST_N
    i = np.arange(n)
    rng = np.random.default_rng(7)
    c = 0x0123_4567_89AB_CDEF
    return {
        "all_equal_i64": ([42] * n, INT64),
        "all_equal_str": (["AAAAAAAAAAAAA123"] * n, STRING),
        # only one high byte varies
        "one_high_byte": ([int(c + ((k % 3) << 40)) for k in i], INT64),
        # only the low byte varies
        "low_byte_i32": ([int(x) for x in rng.integers(0, 200, n)], INT32),
        "prefix_str": ([f"AAAAAAAAAAAAA{int(x):03d}"
                        for x in rng.integers(0, 1000, n)], STRING),
        # proper prefixes of one another and the empty string, length 0..20
        "prefixes": (["abcdefghijklmnopqrst"[:int(k)]
                      for k in rng.integers(0, 21, n)], STRING),
    }


@pytest.mark.parametrize("shape", ["all_equal_i64", "all_equal_str",
                                   "one_high_byte", "low_byte_i32",
                                   "prefix_str", "prefixes"])
def test_constant_digits(shape):
    vals, dt = _const_shapes()[shape]
    rng = np.random.default_rng(11)
    for v in (vals, _with_nulls(vals, rng)):
        for desc in (False, True):
            for nl in (False, True):
                _check([v], [dt], [desc], [nl], shape)


def test_constant_then_varying_key_reuses_diff_word():
    """A key whose every pass is skipped, between keys that need theirs: a
    stale or uncleared varying-bits word would skip a needed pass."""
    n = CONST_N
    rng = np.random.default_rng(12)
    a = [int(x) for x in rng.integers(-2**62, 2**62, n)]
    b = [7] * n
    c = [int(x) for x in rng.integers(0, 5, n)]
    _check([c, b, a], [INT32, INT64, INT64], [False, True, False],
           [False, False, True], "varying/constant/varying")
    _check([b, a], [INT64, INT64], [False, False], [False, False],
           "constant most significant")
    _check([b], [INT64], [True], [True], "constant only")


def test_multi_key_mixed():
    n = 20_000
    rng = np.random.default_rng(13)
    a = _with_nulls([int(x) for x in rng.integers(0, 6, n)], rng)
    words = ["", "a", "ab", "abc", "spark", "rapids", "mi355x", "wörld",
             "AAAAAAAAAAAAA123", "AAAAAAAAAAAAA124"]
    b = _with_nulls([words[int(k)] for k in rng.integers(0, len(words), n)],
                    rng)
    special = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 2.5,
               -2.5]
    c = [special[int(k)] if k < len(special) else float(k)
         for k in rng.integers(0, 12, n)]
    for desc in ([False, True, False], [True, False, True],
                 [True, True, False]):
        for nl in (desc, [not d for d in desc]):
            _check([a, b, c], [INT32, STRING, FLOAT64], desc, nl, "mixed")


def test_string_then_decimal128():
    n = 6000
    rng = np.random.default_rng(14)
    s = _with_nulls([f"k{int(x) % 40:02d}" for x in rng.integers(0, 1000, n)],
                    rng)
    d, _ = _values("decimal128", n, rng)
    d = _with_nulls([d[int(k)] for k in rng.integers(0, 50, n)], rng)
    for desc in ([False, False], [False, True], [True, False]):
        _check([s, d], [STRING, D128], desc, [not x for x in desc],
               "string+decimal128")


def test_no_keys_is_iota():
    from spark_rapids_amd.ops import gpu_backend

    batch = ColumnBatch([_column(list(range(300)), INT32)]).cuda()
    out = gpu_backend.sort_order(batch, [], [], []).cpu().data.numpy()
    assert np.array_equal(out, np.arange(300, dtype=np.int32))


def _topn_rows(enabled, data, n_limit, parts):
    s = sr.Session({"spark.rapids.sql.enabled": enabled})
    df = s.create_dataframe(data, num_partitions=parts)
    return (df.sort("name", "v", "i", descending=[True, False, False])
            .limit(n_limit).collect())


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("n_limit", [7, 20_000])
def test_topn_matches_cpu(n_limit, parts):
    """sort(...).limit(n) gathers only the first n entries of the
    permutation; a limit past the row count keeps every row. One input
    batch is sorted once, several are sorted, truncated and merged."""
    n = 10_000
    rng = np.random.default_rng(15)
    data = {
        "name": [f"item{int(x):04d}" for x in rng.integers(0, 3000, n)],
        "v": [None if x < 0.1 else float(int(x * 50)) for x in rng.random(n)],
        "i": list(range(n)),
    }
    gpu = _topn_rows(True, data, n_limit, parts)
    cpu = _topn_rows(False, data, n_limit, parts)
    assert len(gpu) == min(n_limit, n)
    assert gpu == cpu
