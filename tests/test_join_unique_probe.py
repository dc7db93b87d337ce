"""Single-pass hash-join probe for unique build keys, and the build-once
table: GPU gather maps against the CPU backend over the block-geometry edge
sizes, every join type, match pattern and key shape, plus the non-unique
fallback and the once-per-join build in HashJoinExec."""
import numpy as np
import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, ColumnBatch
from spark_rapids_amd.types import (FLOAT64, INT8, INT16, INT32, INT64,
                                    STRING)

pytestmark = pytest.mark.gpu

HOWS = ["inner", "left", "semi", "anti"]
PATTERNS = ["all", "none", "half", "last_only"]


def _backends():
    from spark_rapids_amd.ops import cpu_backend as cb, gpu_backend as gb
    return cb, gb


def _block_rows():
    """B = HIPDF_BLOCK x JOIN_ITEMS, read off the native block count."""
    _, gb = _backends()
    nb = gb.ext.join_probe_num_blocks
    b = next(b for b in range(1, 1 << 16) if nb(b + 1) == 2)
    assert nb(b) == 1 and nb(2 * b) == 2 and nb(2 * b + 1) == 3
    return b


def _left_sizes():
    b = _block_rows()
    return [0, 1, 63, 64, 65, b - 1, b, b + 1, 2 * b + 17]


def _rows(batch: ColumnBatch):
    return list(zip(*[c.to_pylist() for c in batch.columns]))


def _check(left: ColumnBatch, right: ColumnBatch, lkeys, rkeys, how,
           unique=True):
    """GPU maps (one-call and build/probe split) against the CPU backend.
    Unique build: lmap strictly ascending, maps and gathered rows equal the
    CPU result ordered by lmap. Otherwise: same multiset of pairs."""
    cb, gb = _backends()
    lcpu, rcpu = cb.join_gather_maps(left, right, lkeys, rkeys, how)
    lg, rg = left.cuda(), right.cuda()
    table = gb.join_build_table(rg, rkeys)
    assert table.unique == unique
    results = [gb.join_gather_maps(lg, rg, lkeys, rkeys, how),
               gb.join_probe(table, lg, lkeys, how)]
    cl = lcpu.to_numpy().astype(np.int64)
    cr = rcpu.to_numpy().astype(np.int64) if rcpu is not None else None
    for lgpu, rgpu in results:
        gl = lgpu.to_numpy().astype(np.int64)
        assert (rgpu is None) == (rcpu is None)
        gr = rgpu.to_numpy().astype(np.int64) if rgpu is not None else None
        assert len(gl) == len(cl), (how, len(gl), len(cl))
        if not unique:
            cpairs = sorted(zip(cl, cr if cr is not None else cl))
            gpairs = sorted(zip(gl, gr if gr is not None else gl))
            assert cpairs == gpairs, how
            continue
        assert np.all(np.diff(gl) > 0), (how, "lmap not strictly ascending")
        order = np.argsort(cl, kind="stable")
        assert np.array_equal(gl, cl[order]), how
        if cr is not None:
            assert np.array_equal(gr, cr[order]), how
        # gathered (left ++ right) rows, row for row
        lsorted = Column.from_numpy(cl[order].astype(np.int32), INT32)
        cpu_out = cb.gather(left, lsorted).columns
        gpu_out = gb.gather(lg, lgpu).cpu().columns
        if cr is not None:
            rsorted = Column.from_numpy(cr[order].astype(np.int32), INT32)
            cpu_out = cpu_out + cb.gather(right, rsorted).columns
            gpu_out = gpu_out + gb.gather(rg, rgpu).cpu().columns
        assert _rows(ColumnBatch(gpu_out, len(gl))) == \
            _rows(ColumnBatch(cpu_out, len(cl))), how


def _build_keys(nbuild, rng):
    """Unique keys 3i+7 in shuffled order: key+1 is never a build key."""
    return rng.permutation(nbuild).astype(np.int64) * 3 + 7


def _left_keys(pattern, n, bkeys, rng):
    hit = rng.choice(bkeys, n) if n else np.zeros(0, dtype=np.int64)
    miss = hit + 1
    if pattern == "all":
        return hit
    if pattern == "none":
        return miss
    if pattern == "half":
        return np.where(rng.random(n) < 0.5, hit, miss)
    out = miss.copy()  # only the last row of the last partial block
    if n:
        out[-1] = hit[-1]
    return out


def _int_batches(np_dt, dtype, n, nbuild, pattern, rng):
    bkeys = _build_keys(nbuild, rng)
    lkeys = _left_keys(pattern, n, bkeys, rng)
    left = ColumnBatch([
        Column.from_numpy(lkeys.astype(np_dt), dtype),
        Column.from_numpy(np.arange(n, dtype=np.float64) * 0.5, FLOAT64)], n)
    right = ColumnBatch([
        Column.from_numpy(bkeys.astype(np_dt), dtype),
        Column.from_numpy(np.arange(nbuild, dtype=np.int32) - 5, INT32)],
        nbuild)
    return left, right


@pytest.mark.parametrize("nbuild", [1, 1000])
@pytest.mark.parametrize("how", HOWS)
def test_int32_sizes_and_patterns(how, nbuild):
    """int32 key (inline hash) over every edge size and match pattern; a
    build of 1000 in cap 2048 makes many slots collide."""
    rng = np.random.default_rng(7)
    for n in _left_sizes():
        for pattern in PATTERNS:
            left, right = _int_batches(np.int32, INT32, n, nbuild, pattern,
                                       rng)
            _check(left, right, [0], [0], how)


@pytest.mark.parametrize("how", HOWS)
def test_int64_inline_hash(how):
    """int64 keys with distinct high words (inline hash_long)."""
    rng = np.random.default_rng(8)
    b = _block_rows()
    n, nbuild = 2 * b + 17, 1000
    bkeys = (_build_keys(nbuild, rng) << 33) - (1 << 40)
    lkeys = np.where(rng.random(n) < 0.5, rng.choice(bkeys, n),
                     rng.choice(bkeys, n) + 1)
    left = ColumnBatch([Column.from_numpy(lkeys, INT64),
                        Column.from_numpy(np.arange(n, dtype=np.float64),
                                          FLOAT64)], n)
    right = ColumnBatch([Column.from_numpy(bkeys, INT64),
                         Column.from_numpy(np.arange(nbuild, dtype=np.int32),
                                           INT32)], nbuild)
    _check(left, right, [0], [0], how)


@pytest.mark.parametrize("np_dt,dtype,lo,hi", [
    (np.int8, INT8, -128, 128), (np.int16, INT16, -300, 300)])
@pytest.mark.parametrize("how", HOWS)
def test_narrow_int_sign_extension(how, np_dt, dtype, lo, hi):
    """Negative int8/int16 keys: the inline hash must sign-extend exactly as
    the build-side row hash does, or negative keys land in other slots."""
    rng = np.random.default_rng(9)
    n = _block_rows() + 1
    bkeys = rng.permutation(np.arange(lo, hi, 2))  # even values only
    lkeys = rng.integers(lo, hi, n)
    assert (lkeys < 0).any() and (bkeys < 0).any()
    left = ColumnBatch([Column.from_numpy(lkeys.astype(np_dt), dtype),
                        Column.from_numpy(np.arange(n, dtype=np.float64),
                                          FLOAT64)], n)
    right = ColumnBatch([Column.from_numpy(bkeys.astype(np_dt), dtype),
                         Column.from_numpy(
                             np.arange(len(bkeys), dtype=np.int32), INT32)],
                        len(bkeys))
    _check(left, right, [0], [0], how)


@pytest.mark.parametrize("how", HOWS)
def test_string_key_unique_build(how):
    """String keys use precomputed hashes but still the single-pass probe."""
    rng = np.random.default_rng(10)
    n, nbuild = _block_rows() + 1, 300
    bwords = [f"k{i}" + "x" * (i % 5) for i in range(nbuild)] + [None, None]
    lwords = [None if i % 11 == 0 else
              (bwords[int(rng.integers(nbuild))] if i % 2 else f"miss{i}")
              for i in range(n)]
    left = ColumnBatch([Column.from_pylist(lwords, STRING),
                        Column.from_numpy(np.arange(n, dtype=np.int64),
                                          INT64)], n)
    right = ColumnBatch([Column.from_pylist(bwords, STRING),
                         Column.from_numpy(
                             np.arange(len(bwords), dtype=np.int32), INT32)],
                        len(bwords))
    _check(left, right, [0], [0], how)


@pytest.mark.parametrize("how", HOWS)
def test_two_column_key(how):
    """(int32, int64) key: each column repeats, only the pair is unique."""
    rng = np.random.default_rng(11)
    n = _block_rows() + 1
    a, b = np.divmod(rng.permutation(40 * 25), 25)  # unique (a, b) pairs
    la, lb = rng.integers(0, 45, n), rng.integers(0, 28, n)
    left = ColumnBatch([Column.from_numpy(la.astype(np.int32), INT32),
                        Column.from_numpy(np.arange(n, dtype=np.float64),
                                          FLOAT64),
                        Column.from_numpy(lb.astype(np.int64), INT64)], n)
    right = ColumnBatch([Column.from_numpy(b.astype(np.int64), INT64),
                         Column.from_numpy(a.astype(np.int32), INT32)],
                        len(a))
    _check(left, right, [0, 2], [1, 0], how)


@pytest.mark.parametrize("np_dt,dtype", [(np.int32, INT32),
                                         (np.int64, INT64)])
@pytest.mark.parametrize("how", HOWS)
def test_null_keys(how, np_dt, dtype):
    """Null left keys never match; several null build keys are neither
    duplicates nor matches (their stored values collide with real keys)."""
    rng = np.random.default_rng(12)
    n, nbuild = _block_rows() + 1, 200
    bkeys = rng.permutation(nbuild)
    bvalid = np.ones(nbuild, dtype=bool)
    bvalid[[3, 50, 51, 199]] = False
    bkeys[[3, 50, 51, 199]] = bkeys[0]  # same stored value under the nulls
    lkeys = rng.integers(0, nbuild + 50, n)
    lvalid = rng.random(n) >= 0.2
    left = ColumnBatch([Column.from_numpy(lkeys.astype(np_dt), dtype, lvalid),
                        Column.from_numpy(np.arange(n, dtype=np.float64),
                                          FLOAT64)], n)
    right = ColumnBatch([Column.from_numpy(bkeys.astype(np_dt), dtype,
                                           bvalid),
                         Column.from_numpy(np.arange(nbuild, dtype=np.int32),
                                           INT32)], nbuild)
    _check(left, right, [0], [0], how)


@pytest.mark.parametrize("how", HOWS)
def test_duplicate_build_key_falls_back(how):
    """One duplicated build key: unique is False and the general
    count/scan/fill path gives the CPU backend's multiset of pairs."""
    rng = np.random.default_rng(13)
    n, nbuild = _block_rows() + 1, 1000
    bkeys = _build_keys(nbuild, rng)
    bkeys[-1] = bkeys[0]
    lkeys = np.where(rng.random(n) < 0.5, rng.choice(bkeys, n),
                     rng.choice(bkeys, n) + 1)
    lkeys[:4] = bkeys[0]
    left = ColumnBatch([Column.from_numpy(lkeys.astype(np.int32), INT32),
                        Column.from_numpy(np.arange(n, dtype=np.float64),
                                          FLOAT64)], n)
    right = ColumnBatch([Column.from_numpy(bkeys.astype(np.int32), INT32),
                         Column.from_numpy(np.arange(nbuild, dtype=np.int32),
                                           INT32)], nbuild)
    _check(left, right, [0], [0], how, unique=False)


def _gpu_session():
    # a 1-byte batch goal keeps every left partition its own batch
    return sr.Session({"spark.rapids.sql.batchSizeBytes": 1})


def _frames(session, ldata, rdata, lparts=1):
    return (session.create_dataframe(dict(ldata), num_partitions=lparts),
            session.create_dataframe(dict(rdata)))


def test_full_join_unmatched_right_rows():
    """Full outer through the DataFrame API over 3 left batches: build rows
    no probe row matched come back with null left columns (right_matched
    is written by the single-pass probe)."""
    rng = np.random.default_rng(14)
    n = 2 * _block_rows() + 17
    ldata = {"k": rng.integers(0, 600, n).astype(np.int32),
             "a": np.arange(n, dtype=np.float64)}
    # keys 400..1399 unique; left never reaches 600..1399
    rdata = {"k": (rng.permutation(1000) + 400).astype(np.int32),
             "b": np.arange(1000, dtype=np.int32)}
    lg, rg = _frames(_gpu_session(), ldata, rdata, lparts=3)
    lc, rc = _frames(sr.Session({"spark.rapids.sql.enabled": False}),
                     ldata, rdata, lparts=3)
    q = lg.join(rg, on="k", how="full")
    assert "GpuHashJoin" in q.physical_plan().tree_string()
    gpu = sorted(q.collect(), key=repr)
    cpu = sorted(lc.join(rc, on="k", how="full").collect(), key=repr)
    assert gpu == cpu
    unmatched = [r for r in gpu if r[1] is None]
    seen = set(ldata["k"].tolist())
    assert len(unmatched) == sum(1 for k in rdata["k"].tolist()
                                 if k not in seen) >= 800


@pytest.mark.parametrize("how", ["inner", "left", "anti"])
def test_empty_build_through_exec(how):
    ldata = {"k": np.arange(100, dtype=np.int32),
             "a": np.arange(100, dtype=np.float64)}
    rdata = {"k": np.arange(10, dtype=np.int32),
             "b": np.arange(10, dtype=np.int32)}

    def run(session):
        left, right = _frames(session, ldata, rdata, lparts=2)
        return sorted(left.join(right.filter(sr.col("b") < -1), on="k",
                                how=how).collect(), key=repr)

    gpu = run(_gpu_session())
    assert gpu == run(sr.Session({"spark.rapids.sql.enabled": False}))
    assert len(gpu) == (0 if how == "inner" else 100)


def test_build_once_per_join(monkeypatch):
    """A left child yielding 3 batches probes one table: join_build runs
    once, the single-pass probe three times, the general kernels never."""
    _, gb = _backends()
    calls = {"join_build": 0, "join_probe_unique": 0, "join_count": 0,
             "join_fill": 0}

    def counted(name):
        fn = getattr(gb.ext, name)

        def wrapper(*args):
            calls[name] += 1
            return fn(*args)
        return wrapper

    for name in calls:
        monkeypatch.setattr(gb.ext, name, counted(name))
    rng = np.random.default_rng(15)
    n = 3000
    ldata = {"k": rng.integers(0, 1200, n).astype(np.int32),
             "a": np.arange(n, dtype=np.float64)}
    rdata = {"k": rng.permutation(1000).astype(np.int32),
             "b": np.arange(1000, dtype=np.int32)}
    left, right = _frames(_gpu_session(), ldata, rdata, lparts=3)
    q = left.join(right, on="k")
    assert "GpuHashJoin" in q.physical_plan().tree_string()
    gpu = sorted(q.collect(), key=repr)
    assert calls == {"join_build": 1, "join_probe_unique": 3,
                     "join_count": 0, "join_fill": 0}, calls
    lc, rc = _frames(sr.Session({"spark.rapids.sql.enabled": False}),
                     ldata, rdata, lparts=3)
    assert gpu == sorted(lc.join(rc, on="k").collect(), key=repr)
