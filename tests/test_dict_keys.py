"""Dictionary-coded join strings and the group-by over their codes: a view's
materialised buffers against the eager string gather, join + group-by
queries against the CPU backend over the wave and block edge sizes, the
fallback when the dense bounds fail, and the native dense_gid entry with a
code-table key against numpy.

Value columns hold small integers (also the double one), so every sum is
exact in float64 and rows are compared for equality."""
import struct

import numpy as np
import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, ColumnBatch
from spark_rapids_amd.types import STRING

pytestmark = pytest.mark.gpu

FACT_SIZES = [0, 1, 63, 64, 65, 257, 1000]
DICT_CONF = "spark.rapids.sql.join.dictionaryStrings.enabled"
WORDS = ["", "a", "ab", "", "naïve", "日本語", None, "ab", "z" * 40, "a"]


def _gb():
    from spark_rapids_amd.ops import gpu_backend as gb
    return gb


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def _host(t):
    return t.cpu().numpy()


# ---- materialisation -------------------------------------------------------

def _assert_same_buffers(view, eager, n):
    assert view.size == eager.size == n and view.dtype == eager.dtype
    assert not view.is_materialized
    assert view.nbytes == 4 * n and view.device == "cuda"
    assert not view.is_materialized  # answered without materialising
    assert _host(view.offsets).tobytes() == _host(eager.offsets).tobytes()
    assert _host(view.data).tobytes() == _host(eager.data).tobytes()
    assert view.is_materialized
    assert (view.validity is None) == (eager.validity is None)
    if eager.validity is not None:
        nb = (n + 7) // 8  # the padding behind it is never written
        assert _host(view.validity)[:nb].tobytes() == \
            _host(eager.validity)[:nb].tobytes()
    assert view.to_pylist() == eager.to_pylist()
    assert view.to("cpu").to_pylist() == eager.to_pylist()


@pytest.mark.parametrize("negatives", [False, True])
@pytest.mark.parametrize("null_row", [False, True])
def test_view_materialises_like_eager_gather(null_row, negatives):
    from spark_rapids_amd.column import DictColumn
    gb = _gb()
    words = WORDS if null_row else [w or "" for w in WORDS]
    d = Column.from_pylist(words, STRING).cuda()
    rng = np.random.default_rng(1)
    for n in FACT_SIZES:
        codes = rng.integers(0, len(words), n).astype(np.int32)
        if negatives and n:
            codes[rng.random(n) < 0.3] = -1
            codes[-1] = -1
        idx = _dev(codes)
        eager = gb._gather_col(d, idx, n, negatives)
        view = DictColumn(d, idx, n, negatives)
        if not null_row and not negatives:
            assert view.validity is None and not view.is_materialized
        _assert_same_buffers(view, eager, n)


def test_zero_row_view():
    from spark_rapids_amd.column import DictColumn
    gb = _gb()
    d = Column.from_pylist(WORDS, STRING).cuda()
    idx = _dev(np.zeros(0, dtype=np.int32))
    view = DictColumn(d, idx, 0, True)
    _assert_same_buffers(view, gb._gather_col(d, idx, 0, True), 0)
    assert view.to_pylist() == []


def test_view_gathered_twice_and_sliced():
    """Gathers of a view move only the codes; views that shared their codes
    still share them; the end result equals the eager chain."""
    from spark_rapids_amd.column import DictColumn
    from spark_rapids_amd.plan.physical import _slice_rows
    gb = _gb()
    d1 = Column.from_pylist(WORDS, STRING).cuda()
    d2 = Column.from_pylist([w and w[::-1] for w in WORDS], STRING).cuda()
    rng = np.random.default_rng(2)
    n = 1000
    rmap = Column.from_numpy(
        rng.integers(-1, len(WORDS), n).astype(np.int32)).cuda()
    first = gb.gather_dict(ColumnBatch([d1, d2], len(WORDS)), rmap, True)
    eager = gb.gather(ColumnBatch([d1, d2], len(WORDS)), rmap, negatives=True)
    assert first.columns[0].codes is first.columns[1].codes
    for step, m in enumerate([257, 65]):
        idx = rng.integers(-1 if step else 0, first.num_rows, m)
        icol = Column.from_numpy(idx.astype(np.int32)).cuda()
        first = gb.gather(first, icol, negatives=bool(step))
        eager = gb.gather(eager, icol, negatives=bool(step))
    first, eager = _slice_rows(first, 3, 64), _slice_rows(eager, 3, 64)
    a, b = first.columns
    assert isinstance(a, DictColumn) and isinstance(b, DictColumn)
    assert a.codes is b.codes and a.dictionary is d1 and b.dictionary is d2
    for v, e in zip(first.columns, eager.columns):
        _assert_same_buffers(v, e, 61)


def test_build_side_views_compose():
    """A gather of a dictionary whose own rows are views composes codes."""
    from spark_rapids_amd.column import DictColumn
    gb = _gb()
    d = Column.from_pylist(WORDS, STRING).cuda()
    inner = Column.from_numpy(np.array([9, -1, 4, 6, 0], np.int32)).cuda()
    outer = Column.from_numpy(np.array([1, 0, -1, 3, 2, 2], np.int32)).cuda()
    mid = gb.gather_dict(ColumnBatch([d], len(WORDS)), inner, True)
    out = gb.gather_dict(mid, outer, True).columns[0]
    assert isinstance(out, DictColumn) and out.dictionary is d
    assert not mid.columns[0].is_materialized
    assert out.to_pylist() == [None, "a", None, None, "naïve", "naïve"]


def test_concat_keeps_views_over_one_dictionary():
    from spark_rapids_amd.column import DictColumn
    gb = _gb()
    d = Column.from_pylist(WORDS, STRING).cuda()
    other = Column.from_pylist(WORDS, STRING).cuda()
    m1 = Column.from_numpy(np.array([1, 2, -1], np.int32)).cuda()
    m2 = Column.from_numpy(np.array([5, 0], np.int32)).cuda()
    b1 = gb.gather_dict(ColumnBatch([d], len(WORDS)), m1, True)
    b2 = gb.gather_dict(ColumnBatch([d], len(WORDS)), m2, False)
    cat = gb.concat_batches([b1, b2]).columns[0]
    assert isinstance(cat, DictColumn) and not b1.columns[0].is_materialized
    assert cat.to_pylist() == ["a", "ab", None, "日本語", ""]
    b3 = gb.gather_dict(ColumnBatch([other], len(WORDS)), m2, False)
    mixed = gb.concat_batches([b1, b3]).columns[0]
    assert not isinstance(mixed, DictColumn)
    assert mixed.to_pylist() == ["a", "ab", None, "日本語", ""]


# ---- join + group-by against the CPU backend ------------------------------

def _dims(na=300, nb=7, nc=1):
    """dim a: duplicate strings, two string columns and a NULL string; dim
    b: few rows; dim c: `nc` rows (1 is the smallest dimension)."""
    a = {"ak": np.arange(na, dtype=np.int32),
         "a_name": [None if k % 11 == 5 else f"n{k % 7}é" for k in range(na)],
         "a_cat": [f"c{k % 3}" for k in range(na)]}
    b = {"bk": np.arange(nb, dtype=np.int32),
         "b_state": ["", "x", "yy", "x", "Ω", "yy", "q"][:nb]}
    c = {"ck": np.arange(nc, dtype=np.int32),
         "c_name": [f"s{k % 2}" for k in range(nc)]}
    return a, b, c


def _fact(n, rng, na=300, nb=7, nc=1, miss=0):
    return {"fa": rng.integers(0, na + miss, n).astype(np.int32),
            "fb": rng.integers(0, nb, n).astype(np.int32),
            "fc": rng.integers(0, nc, n).astype(np.int32),
            "m": rng.integers(3, 6, n).astype(np.int32),
            "v": rng.integers(0, 10, n).astype(np.int64),
            "w": rng.integers(0, 10, n).astype(np.float64)}


def _sessions(on=True):
    return (sr.Session({DICT_CONF: on}),
            sr.Session({"spark.rapids.sql.enabled": False}))


def _run(session, fact, dims, query):
    n = len(fact["v"])
    f = session.create_dataframe(dict(fact),
                                 num_partitions=2 if n >= 64 else 1)
    ds = [session.create_dataframe(dict(d)) for d in dims]
    return sorted(query(f, *ds).collect(), key=repr)


def _agree(query, sizes=FACT_SIZES, on=True, **shape):
    """GPU rows == CPU rows for every fact size; returns the GPU rows of
    the largest size."""
    gpu_s, cpu_s = _sessions(on)
    rng = np.random.default_rng(3)
    dims = _dims(**{k: v for k, v in shape.items() if k != "miss"})
    rows = None
    for n in sizes:
        fact = _fact(n, rng, **shape)
        rows = _run(gpu_s, fact, dims, query)
        assert rows == _run(cpu_s, fact, dims, query), n
    return rows


def _watch_group_by(monkeypatch):
    """Record what every backend group_by_aggregate call is handed."""
    gb = _gb()
    seen = []
    real = gb.group_by_aggregate

    def wrapper(batch, key_idx, aggs, sel=None):
        seen.append({"keys": [batch.columns[i] for i in key_idx],
                     "rows": batch.num_rows, "sel": sel is not None})
        return real(batch, key_idx, aggs, sel=sel)

    monkeypatch.setattr(gb, "group_by_aggregate", wrapper)
    return seen


def _count_calls(monkeypatch, *names):
    gb = _gb()
    calls = {n: [] for n in names}
    for name in names:
        fn = getattr(gb.ext, name)

        def wrapper(*args, _fn=fn, _name=name):
            calls[_name].append(args)
            return _fn(*args)

        monkeypatch.setattr(gb.ext, name, wrapper)
    return calls


AGGS = (sr.sum_(sr.col("v")), sr.sum_(sr.col("w")), sr.count_star())


def test_one_key_duplicate_dictionary_strings():
    rows = _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
                  .group_by("a_name").agg(*AGGS))
    assert len(rows) == 8  # seven names and the NULL string


def test_two_keys_of_one_dimension_grouped_jointly(monkeypatch):
    calls = _count_calls(monkeypatch, "gb_build")
    seen = _watch_group_by(monkeypatch)
    gpu_s, _ = _sessions()
    fact = _fact(1000, np.random.default_rng(3))
    rows = _run(gpu_s, fact, _dims(),
                lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
                .group_by("a_name", "a_cat").agg(*AGGS))
    assert len(rows) == 24
    # one joint build over the 300 dictionary rows per fact batch, plus the
    # merge of the partial results: never one per key, never at fact scale
    partials = [s for s in seen if s["rows"] >= 500]
    builds = [args[-2] for args in calls["gb_build"]]
    assert partials and builds.count(300) == len(partials)
    assert all(n == 300 or n <= 24 * len(partials) for n in builds)
    _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
           .group_by("a_name", "a_cat").agg(*AGGS))


def test_two_dimensions_and_an_integer_key():
    rows = _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
                  .join(b, on="fb", right_on=["bk"])
                  .group_by("a_name", "m", "b_state").agg(*AGGS))
    assert {r[1] for r in rows} == {3, 4, 5}
    assert {r[2] for r in rows} == {"", "x", "yy", "Ω", "q"}


def test_left_join_misses_and_null_string_make_one_group():
    """Fact keys past the dimension miss (-1 codes); the dictionary also
    holds NULL strings: both land in the one NULL group."""
    def q(f, a, b, c):
        return f.join(a, on="fa", right_on=["ak"], how="left") \
            .group_by("a_name").agg(*AGGS)

    rows = _agree(q, miss=100)
    nulls = [r for r in rows if r[0] is None]
    assert len(nulls) == 1 and len(rows) == 8
    # its count is the misses plus the NULL strings of the last fact table
    rng = np.random.default_rng(3)
    for n in FACT_SIZES:
        fact = _fact(n, rng, miss=100)
    missed = int((fact["fa"] >= 300).sum())
    null_str = int(((fact["fa"] < 300) & (fact["fa"] % 11 == 5)).sum())
    assert missed and null_str and nulls[0][3] == missed + null_str
    # two string keys of the left-joined dimension: a miss makes both NULL
    rows = _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"],
                                            how="left")
                  .group_by("a_cat", "a_name").agg(*AGGS), miss=100)
    assert sum(1 for r in rows if r[0] is None and r[1] is None) == 1


def test_fused_filter_selection(monkeypatch):
    """A predicate over both sides stays above the join, where the
    aggregate fuses it into a selection vector over the coded keys."""
    from spark_rapids_amd.column import DictColumn
    seen = _watch_group_by(monkeypatch)
    _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
           .filter(sr.col("v") + sr.col("ak") > 150)
           .group_by("a_name", "m").agg(*AGGS))
    fused = [s for s in seen if s["sel"]]
    assert fused and all(isinstance(s["keys"][0], DictColumn)
                         and not s["keys"][0].is_materialized for s in fused)


def test_filter_leaves_no_rows(monkeypatch):
    seen = _watch_group_by(monkeypatch)
    rows = _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
                  .filter(sr.col("v") + sr.col("ak") > 100000)
                  .group_by("a_name").agg(*AGGS))
    assert rows == [] and any(s["sel"] for s in seen)


def test_keys_regathered_through_two_further_joins(monkeypatch):
    from spark_rapids_amd.column import DictColumn
    seen = _watch_group_by(monkeypatch)
    _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
           .join(b, on="fb", right_on=["bk"])
           .join(c, on="fc", right_on=["ck"])
           .group_by("a_name", "a_cat", "c_name").agg(*AGGS), nc=2)
    first = next(s for s in seen if s["rows"] >= 500)
    assert all(isinstance(k, DictColumn) and not k.is_materialized
               for k in first["keys"])
    assert first["keys"][0].codes is first["keys"][1].codes


@pytest.mark.parametrize("count_all", [True, False])
def test_live_flags_with_and_without_count_all(monkeypatch, count_all):
    calls = _count_calls(monkeypatch, "dense_gid", "gb_collect_count")
    aggs = AGGS if count_all else AGGS[:2]
    _agree(lambda f, a, b, c: f.join(a, on="fa", right_on=["ak"])
           .group_by("a_name", "m").agg(*aggs))
    fact_scale = [a for a in calls["dense_gid"] if a[5] >= 500]
    assert fact_scale
    # live flags exactly when no count_all aggregate carries the counts
    assert all((a[4] == 0) == count_all for a in fact_scale)
    assert not calls["gb_collect_count"]


def test_fallback_when_dense_bounds_fail(monkeypatch):
    """300 x 300 distinct strings over 1000 rows: 90 000 ids exceed
    max(65536, 4n), so the hash path runs over the materialised strings."""
    from spark_rapids_amd.column import DictColumn
    calls = _count_calls(monkeypatch, "gb_build", "dense_gid")
    seen = _watch_group_by(monkeypatch)
    a = {"ak": np.arange(300, dtype=np.int32),
         "a_name": [f"a{k}" for k in range(300)]}
    b = {"bk": np.arange(300, dtype=np.int32),
         "b_name": [f"b{k}" for k in range(300)]}
    rng = np.random.default_rng(4)
    fact = {"fa": rng.integers(0, 300, 1000).astype(np.int32),
            "fb": rng.integers(0, 300, 1000).astype(np.int32),
            "v": rng.integers(0, 10, 1000).astype(np.int64),
            "w": rng.integers(0, 10, 1000).astype(np.float64)}

    def q(f, da, db):
        return f.join(da, on="fa", right_on=["ak"]) \
            .join(db, on="fb", right_on=["bk"]) \
            .group_by("a_name", "b_name").agg(*AGGS)

    gpu_s, cpu_s = _sessions()
    rows = _run(gpu_s, fact, (a, b), q)
    assert rows == _run(cpu_s, fact, (a, b), q)
    assert not calls["dense_gid"]
    # every group-by over view keys built its table over all fact rows
    coded = [s for s in seen if isinstance(s["keys"][0], DictColumn)]
    builds = [args[-2] for args in calls["gb_build"]]
    assert coded and sum(s["rows"] for s in coded) == 1000
    assert all(s["rows"] in builds and s["keys"][0].is_materialized
               for s in coded)


def test_join_strings_stay_unmaterialised(monkeypatch):
    """The point of the change: after collect() the join output's string
    columns were never materialised; with the conf off the join hands out
    plain (materialised) columns, and both settings give the same rows."""
    from spark_rapids_amd.column import DictColumn
    calls = _count_calls(monkeypatch, "gather_str_lens", "murmur3_str")
    seen = _watch_group_by(monkeypatch)

    def q(f, a, b, c):
        return f.join(a, on="fa", right_on=["ak"]) \
            .join(b, on="fb", right_on=["bk"]) \
            .group_by("a_name", "a_cat", "b_state").agg(*AGGS)

    on = _agree(q, sizes=[1000], on=True)
    partial = [s for s in seen if s["rows"] >= 500]
    assert partial
    for s in partial:
        assert all(isinstance(k, DictColumn) and not k.is_materialized
                   for k in s["keys"])
    # strings were touched at dimension and result scale only
    assert all(a[3] < 500 for a in calls["gather_str_lens"])
    assert all(a[5] <= 300 for a in calls["murmur3_str"])
    seen.clear()
    off = _agree(q, sizes=[1000], on=False)
    partial = [s for s in seen if s["rows"] >= 500]
    assert partial
    for s in partial:
        assert not any(isinstance(k, DictColumn) for k in s["keys"])
    assert on == off


# ---- native entry ----------------------------------------------------------

@pytest.mark.parametrize("use_sel", [False, True])
def test_dense_gid_code_table_against_numpy(use_sel):
    import torch
    gb = _gb()
    rng = np.random.default_rng(5)
    nd, g = 37, 5
    table = rng.integers(0, g, nd).astype(np.int32)
    t_table = _dev(table)
    for rows in FACT_SIZES:
        idx = rng.integers(-1, nd, rows).astype(np.int32)
        if rows:
            idx[-1] = -1
        ints = rng.integers(-3, 4, rows).astype(np.int16)
        sel = None
        n = rows
        if use_sel:
            sel = np.flatnonzero(rng.random(rows) < 0.5).astype(np.int32)
            n = len(sel)
        t_idx, t_ints = _dev(idx), _dev(ints)
        t_sel = _dev(sel) if use_sel else None
        # HipdfDenseKey: the code table (range g, NULL slot g) x an int16 key
        blob = struct.pack("<iiqqqqqq", 3, 0, t_table.data_ptr(), 0, 0, g, 7,
                           t_idx.data_ptr()) + \
            struct.pack("<iiqqqqqq", 2, 0, t_ints.data_ptr(), 0, -3, 7, 1, 0)
        desc = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        gid = torch.full((max(n, 1),), -7, dtype=torch.int32,
                         device="cuda")[:n]
        live = torch.zeros((g + 1) * 7, dtype=torch.uint8, device="cuda")
        gb.ext.dense_gid(desc.data_ptr(), 2, gb._ptr(t_sel), gid.data_ptr(),
                         live.data_ptr(), n, gb._stream())
        take = sel if use_sel else np.arange(rows)
        code = np.where(idx[take] >= 0, table[np.maximum(idx[take], 0)], g)
        want = code.astype(np.int64) * 7 + (ints[take].astype(np.int64) + 3)
        assert np.array_equal(_host(gid), want.astype(np.int32)), rows
        want_live = np.zeros((g + 1) * 7, dtype=np.uint8)
        want_live[want] = 1
        assert np.array_equal(_host(live), want_live), rows
        # no live pointer: same ids
        gid2 = torch.empty_like(gid)
        gb.ext.dense_gid(desc.data_ptr(), 2, gb._ptr(t_sel), gid2.data_ptr(),
                         0, n, gb._stream())
        assert np.array_equal(_host(gid2), _host(gid))
