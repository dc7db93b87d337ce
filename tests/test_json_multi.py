"""Several JSON paths over one column in one parse per row
(get_json_object_multi), json_tuple on top of it, and the fusion of
get_json_object calls in GPU projects. The corpora are those of
test_json_path.py."""
import os
import shutil
import subprocess

import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, DType, col
from spark_rapids_amd.expr import json_path
from spark_rapids_amd.expr.json_path import KEY, MAX_FUSED_PATHS
from spark_rapids_amd.ops import cpu_backend

from .test_json_path import (DUPS, GEN_PATHS, HAND, P16, clean_corpus,
                            messy_corpus)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "native", "hipdf")

GROUPS = [
    # shared prefixes, one path's result inside another's
    ["$.a", "$.a.b", "$.a[1]", "$.a[1].b"],
    # the root, a miss, the deepest allowed path, eight paths
    ["$", "$.s", "$.missing", "$['k k']", "$.a[99]", "$.b.c[0]", "$[0].a",
     P16],
    ["$.a", "$.s"],
    ["$.a", "$.a"],
]


def _cpu_answers(rows, path):
    return cpu_backend.get_json_object(
        Column.from_pylist(rows, DType.string()), path).to_pylist()


def _chunks(group):
    return [group[i:i + MAX_FUSED_PATHS]
            for i in range(0, len(group), MAX_FUSED_PATHS)]


def test_max_fused_paths_mirrors_the_header():
    import re

    with open(os.path.join(NATIVE, "kernels", "json_path.h")) as f:
        m = re.search(r"constexpr int kMaxFusedPaths = (\d+);", f.read())
    assert int(m.group(1)) == MAX_FUSED_PATHS


# ---- the device scanner, run on the host ------------------------------------

def _hex(s):
    return "x" + s.encode("utf-8").hex()


def _write_cases(path, group, rows, answers):
    """answers[k][r]: a string, None for NULL, or ... for `not compared`."""
    with open(path, "w") as f:
        f.write(f"{len(group)}\n")
        for p in group:
            steps = json_path.parse(p)
            f.write(f"{len(steps)}\n")
            for kind, arg in steps:
                f.write(f"k {_hex(arg)}\n" if kind == KEY else f"i {arg}\n")
        for r, doc in enumerate(rows):
            cells = []
            for k in range(len(group)):
                want = answers[k][r]
                cells.append("?" if want is ... else
                             "-" if want is None else _hex(want))
            f.write(f"{_hex(doc)} {' '.join(cells)}\n")


@pytest.fixture(scope="module")
def multi_host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("jm") / "json_multi_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall",
                    "-fsanitize=address,undefined",
                    "-I" + os.path.join(NATIVE, "kernels"),
                    os.path.join(NATIVE, "tests", "json_multi_host_test.cpp"),
                    "-o", exe], check=True)
    return exe


def test_multi_scanner_on_host_equals_single_scanner(multi_host_exe,
                                                     tmp_path):
    common = [r for r in HAND if r is not None] + clean_corpus() + \
        messy_corpus()
    dups = [doc for doc, _ in DUPS]
    rows = common + dups
    nchunk = 0
    for group in GROUPS:
        for chunk in _chunks(group):
            answers = []
            recorded = cpu_backend.get_json_object_multi(
                Column.from_pylist(rows, DType.string()),
                [json_path.parse(p) for p in chunk])
            for p, column in zip(chunk, recorded):
                got = column.to_pylist()
                # a duplicated key inside the result is the documented
                # divergence: bytes are compared only where the path is
                # listed for that document
                for i, (_, listed) in enumerate(DUPS):
                    if p not in listed:
                        got[len(common) + i] = ...
                answers.append(got)
            cases = str(tmp_path / f"cases{nchunk}.txt")
            nchunk += 1
            _write_cases(cases, chunk, rows, answers)
            run = subprocess.run([multi_host_exe, cases],
                                 capture_output=True, text=True)
            print(chunk, run.stdout[-400:])
            assert run.returncode == 0, (chunk, run.stdout[-2000:],
                                         run.stderr[-2000:])
            assert f"rows {len(rows)} " in run.stdout


# ---- json_tuple on the host -------------------------------------------------

TUPLE_DOC = '{"a":1,"b":"x","a.b":2,"it\'s":3,"":4,"é":5}'
TUPLE_FIELDS = ["a", "b", "a.b", "it's", "", "é", "missing", None]
TUPLE_WANT = ["1", "x", "2", "3", "4", "5", None, None]


def test_json_tuple_literal_answers(cpu_session):
    rows = [TUPLE_DOC, '[{"a":1}]', '"a"', '{"a":1', None]
    df = cpu_session.create_dataframe({"j": rows},
                                      dtypes={"j": DType.string()})
    out = df.select(sr.json_tuple(col("j"), *TUPLE_FIELDS)).to_pydict()
    assert list(out) == [f"c{i}" for i in range(len(TUPLE_FIELDS))]
    for i, want in enumerate(TUPLE_WANT):
        # a non-object root, an invalid document and a NULL row: all NULL
        assert out[f"c{i}"] == [want, None, None, None, None], i
    assert df.select(col("j").json_tuple("a", "b")).to_pydict() == \
        {"c0": out["c0"], "c1": out["c1"]}
    with pytest.raises(ValueError):
        sr.json_tuple(col("j"))


def test_json_tuple_names_are_keys_not_paths(cpu_session):
    df = cpu_session.create_dataframe(
        {"j": ['{"a":{"b":7},"x":[8],"a.b":1,"x[0]":2,"$":3}']})
    out = df.select(sr.json_tuple(col("j"), "a.b", "x[0]", "$", "a")
                    ).to_pydict()
    assert out == {"c0": ["1"], "c1": ["2"], "c2": ["3"], "c3": ['{"b":7}']}


def test_json_tuple_sql(cpu_session):
    from spark_rapids_amd.sql.parser import SqlError

    df = cpu_session.create_dataframe({"j": [TUPLE_DOC, None], "k": [1, 2]})
    cpu_session.register("tjt", df)
    got = cpu_session.sql("select json_tuple(j, 'a', 'b') from tjt"
                          ).to_pydict()
    assert got == {"c0": ["1", None], "c1": ["x", None]}
    got = cpu_session.sql(
        "select k, json_tuple(j, 'a.b', NULL, 'it''s') AS (x, y, z) from tjt"
    ).to_pydict()
    assert got == {"k": [1, 2], "x": ["2", None], "y": [None, None],
                   "z": ["3", None]}
    # one field may be named without parentheses
    got = cpu_session.sql("select json_tuple(j, 'b') AS x, k from tjt"
                          ).to_pydict()
    assert got == {"x": ["x", None], "k": [1, 2]}
    with pytest.raises(SqlError, match="json_tuple gives 2 columns"):
        cpu_session.sql("select json_tuple(j, 'a', 'b') AS x from tjt")
    for bad in ("select json_tuple(j, k) from tjt",
                "select json_tuple(j, 'a', 1) from tjt",
                "select json_tuple(j, concat_ws('', 'a')) from tjt",
                "select json_tuple(j) from tjt",
                "select json_tuple(j, 'a', 'b') AS (x) from tjt"):
        with pytest.raises(SqlError):
            cpu_session.sql(bad)


def test_select_spreads_lists(cpu_session):
    df = cpu_session.create_dataframe({"j": [TUPLE_DOC], "k": [1]})
    es = sr.json_tuple(col("j"), "a", "b")
    assert df.select("k", es, col("j")).to_pydict() == \
        df.select("k", *es, col("j")).to_pydict()
    assert df.select(tuple(es)).to_pydict() == {"c0": ["1"], "c1": ["x"]}


def test_cpu_backend_multi_equals_single():
    rows = HAND + messy_corpus()[:100]
    c = Column.from_pylist(rows, DType.string())
    group = GROUPS[0] + ["$.a["]
    got = cpu_backend.get_json_object_multi(
        c, [json_path.parse(p) for p in group])
    for p, g in zip(group, got):
        assert g.to_pylist() == _cpu_answers(rows, p), p
    assert got[-1].to_pylist() == [None] * len(rows)


def test_docs_list_json_tuple_and_conf():
    from spark_rapids_amd.tools import docgen

    ops_doc = docgen.supported_ops_doc()
    assert "| JsonTuple |" in ops_doc
    assert "share one parse" in ops_doc
    key = "spark.rapids.sql.json.combinePaths.enabled"
    assert key in sr.help_doc()
    with open(os.path.join(REPO, "docs", "configs.md")) as f:
        assert key in f.read()
    with open(os.path.join(REPO, "docs", "supported_ops.md")) as f:
        assert f.read() == ops_doc


def test_project_groups_paths_by_child():
    from spark_rapids_amd.expr.expressions import (CaseWhen, exists, lit)
    from spark_rapids_amd.plan.physical import _json_path_groups

    j = col("j")
    a, s, b = (j.get_json_object(p) for p in ("$.a", "$.s", "$.b"))
    inner = col("x").get_json_object("$.a")
    exprs = [a.alias("a"), s.cast(DType.int64()),
             CaseWhen([(col("k") > 0, b)], lit("no")), inner,
             # its row set is the array's elements: never fused
             exists(col("arr"), lambda v: v.get_json_object("$.a") ==
                    j.get_json_object("$.z"))]
    groups = _json_path_groups(exprs)
    assert [[n.path for n in g] for g in groups] == [["$.a", "$.s", "$.b"]]
    # one path twice is still one parse of its own
    assert _json_path_groups([a, j.get_json_object("$.a")]) == []
    assert len(_json_path_groups(sr.json_tuple(j, "a", "b"))) == 1


# ---- GPU --------------------------------------------------------------------

def _steps(group):
    return [None if p is None else json_path.parse(p) for p in group]


def _check_group(gpu_backend, rows, group):
    c = Column.from_pylist(rows, DType.string()).cuda()
    got = gpu_backend.get_json_object_multi(c, _steps(group))
    assert len(got) == len(group)
    for p, g in zip(group, got):
        assert g.size == len(rows)
        if p is None:
            assert g.to_pylist() == [None] * len(rows)
            continue
        assert g.to_pylist() == \
            gpu_backend.get_json_object(c, p).to_pylist(), p
        assert g.to_pylist() == _cpu_answers(rows, p), p
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GROUPS)))
def test_gpu_multi_hand_corpus(gi):
    from spark_rapids_amd.ops import gpu_backend

    rows = (HAND * 3)[:193]  # three waves plus one lane
    assert len(rows) == 193 and None in rows
    _check_group(gpu_backend, rows, GROUPS[gi])


@pytest.mark.gpu
def test_gpu_multi_tiny_inputs_and_malformed_path():
    from spark_rapids_amd.ops import gpu_backend

    for group in GROUPS:
        _check_group(gpu_backend, ['{"a":[10,{"b":"x"}],"s":"q\\"q"}'], group)
        got = gpu_backend.get_json_object_multi(
            Column.from_pylist([], DType.string()).cuda(), _steps(group))
        assert [g.size for g in got] == [0] * len(group)
    rows = (HAND * 3)[:193]
    _check_group(gpu_backend, rows, ["$.a", None, "$.s", None])
    _check_group(gpu_backend, rows, [None, "$.a"])
    _check_group(gpu_backend, rows, [None])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 2, 3, MAX_FUSED_PATHS,
                                  MAX_FUSED_PATHS + 1])
def test_gpu_multi_group_sizes(size):
    from spark_rapids_amd.ops import gpu_backend

    pool = GEN_PATHS + ["$.a[99]"]
    assert size <= len(pool)
    rows = messy_corpus()[:150] + [r for r in HAND if r is not None][:50]
    _check_group(gpu_backend, rows, pool[:size])


@pytest.mark.gpu
def test_gpu_multi_same_path_twice():
    from spark_rapids_amd.ops import gpu_backend

    rows = (HAND * 3)[:193]
    a, s, a2 = _check_group(gpu_backend, rows, ["$.a", "$.s", "$.a"])
    assert a.to_pylist() == a2.to_pylist()


@pytest.mark.gpu
def test_gpu_multi_columns_are_ordinary_string_columns():
    # what consumers of a device string column rely on: offsets that start
    # at 0 and end at data.numel(), whichever path of the group it is, with
    # or without rows that the host answered
    from spark_rapids_amd.ops import gpu_backend

    rows = (HAND * 3)[:193]
    for group in (GROUPS[0], GROUPS[1], ["$.missing", "$.a[99]"]):
        for g in _check_group(gpu_backend, rows, group):
            assert int(g.offsets[0].item()) == 0
            assert int(g.offsets[-1].item()) == g.data.numel()
            assert g.offsets.numel() == len(rows) + 1


@pytest.mark.gpu
def test_gpu_multi_columns_concatenate_on_device():
    from spark_rapids_amd import ColumnBatch
    from spark_rapids_amd.ops import gpu_backend

    parts = [(HAND * 3)[:193], messy_corpus()[:70], ['{"a":1e2,"s":"x"}']]
    group = GROUPS[0] + ["$.s"]
    batches = [ColumnBatch(gpu_backend.get_json_object_multi(
        Column.from_pylist(rows, DType.string()).cuda(), _steps(group)))
        for rows in parts]
    whole = gpu_backend.concat_batches(batches)
    everything = [r for rows in parts for r in rows]
    for p, c in zip(group, whole.columns):
        assert c.to_pylist() == _cpu_answers(everything, p), p


@pytest.mark.gpu
def test_gpu_fused_batches_meet_in_a_sort(gpu_session, cpu_session,
                                          gpu_calls):
    rows = messy_corpus()[:120] + [r for r in HAND if r is not None][:40]
    half = len(rows) // 2
    paths = ["$.a", "$.s", "$.a[1]", "$.b.c[0]"]
    out = []
    for s in (cpu_session, gpu_session):
        a = s.create_dataframe({"i": list(range(half)), "j": rows[:half]},
                               dtypes={"j": DType.string()})
        b = s.create_dataframe(
            {"i": list(range(half, len(rows))), "j": rows[half:]},
            dtypes={"j": DType.string()})
        q = a.union(b).select(
            col("i"), *[col("j").get_json_object(p).alias(f"p{k}")
                        for k, p in enumerate(paths)]
        ).sort("i", descending=True)
        out.append(q.to_pydict())
    assert out[0] == out[1]
    assert out[0]["i"][0] == len(rows) - 1
    # one fused call per input batch: two batches reached the sort
    assert gpu_calls == {"multi": 2, "single": 0}


@pytest.mark.gpu
def test_gpu_multi_column_slice_with_nonzero_first_offset():
    from spark_rapids_amd.ops import gpu_backend

    rows = [r for r in HAND if r is not None][:60]
    full = Column.from_pylist(rows, DType.string()).cuda()
    k = 7
    part = Column(DType.string(), full.size - k, full.data, None,
                  full.offsets[k:], 0)
    assert int(part.offsets[0].item()) > 0
    group = ["$.a", "$.a[1].b", "$.s", "$"]
    got = gpu_backend.get_json_object_multi(part, _steps(group))
    for p, g in zip(group, got):
        assert g.to_pylist() == _cpu_answers(rows[k:], p), p


def _select_all(session, rows, paths):
    df = session.create_dataframe({"j": rows}, dtypes={"j": DType.string()})
    return df.select(*[col("j").get_json_object(p).alias(f"p{i}")
                       for i, p in enumerate(paths)]).to_pydict()


@pytest.fixture
def host_calls(monkeypatch):
    """(steps or path, rows) of every column handed to the host backend."""
    calls = []
    real_steps = cpu_backend.get_json_object_steps
    real_path = cpu_backend.get_json_object

    def rec_steps(c, steps):
        calls.append((list(steps), c.size))
        return real_steps(c, steps)

    def rec_path(c, path):
        calls.append((path, c.size))
        return real_path(c, path)

    def arm():
        monkeypatch.setattr(cpu_backend, "get_json_object_steps", rec_steps)
        monkeypatch.setattr(cpu_backend, "get_json_object", rec_path)
        return calls

    return arm


@pytest.fixture
def gpu_calls(monkeypatch):
    """Counts the GPU backend's fused and single-path calls."""
    from spark_rapids_amd.ops import gpu_backend

    counts = {"multi": 0, "single": 0}
    real_multi = gpu_backend.get_json_object_multi
    real_single = gpu_backend.get_json_object

    def multi(c, steps_list):
        counts["multi"] += 1
        return real_multi(c, steps_list)

    def single(c, path):
        counts["single"] += 1
        return real_single(c, path)

    monkeypatch.setattr(gpu_backend, "get_json_object_multi", multi)
    monkeypatch.setattr(gpu_backend, "get_json_object", single)
    return counts


@pytest.mark.gpu
def test_gpu_fused_clean_corpus_never_asks_host(gpu_session, cpu_session,
                                                host_calls, gpu_calls):
    rows = clean_corpus()
    want = _select_all(cpu_session, rows, GEN_PATHS)
    calls = host_calls()
    got = _select_all(gpu_session, rows, GEN_PATHS)
    assert calls == [], calls
    assert gpu_calls == {"multi": 1, "single": 0}
    for i, p in enumerate(GEN_PATHS):
        for r, (g, w) in enumerate(zip(got[f"p{i}"], want[f"p{i}"])):
            assert g == w, (p, rows[r], g, w)


@pytest.mark.gpu
def test_gpu_fused_flagged_rows_go_to_host_per_path(gpu_session, cpu_session,
                                                    host_calls):
    U = chr(92) + "u"
    rows = ['{"a":1e2,"s":"x"}',
            '{"a":{"' + U + '0062":1},"s":2}',
            '{"a":1,"s":"y","z":NaN}',
            '{"a":3,"s":[12.50]}']
    group = ["$.a", "$.s", "$.a.b"]
    want = _select_all(cpu_session, rows, group)
    calls = host_calls()
    got = _select_all(gpu_session, rows, group)
    # rows 0,1,2 / rows 2,3 / rows 1,2
    assert calls == [(json_path.parse("$.a"), 3), (json_path.parse("$.s"), 2),
                     (json_path.parse("$.a.b"), 2)], calls
    assert got == want
    assert want["p0"][0] == "100.0" and want["p1"][3] == "[12.5]"


def _fusion_frame(session):
    rows = ['{"a":1,"n":"12","s":"x","b":{"c":[5,6]}}',
            '{"a":[2],"n":"-7","s":"y","b":{"c":["z"]}}',
            None,
            '{"a":"t","n":"3"']
    df = session.create_dataframe(
        {"j": rows, "j2": list(reversed(rows)), "k": [1, 0, 1, 0]},
        dtypes={"j": DType.string(), "j2": DType.string()})
    return df


def _fusion_exprs(name):
    from spark_rapids_amd.expr.expressions import CaseWhen, lit

    j = col(name)
    return [j.get_json_object("$.a").alias(name + "a"),
            j.get_json_object("$.n").cast(DType.int64()).alias(name + "n"),
            CaseWhen([(col("k") > 0,
                       j.get_json_object("$.b.c[0]").cast(DType.int64()))],
                     lit(-1)).alias(name + "c"),
            j.get_json_object("$.s").alias(name + "s")]


@pytest.mark.gpu
def test_gpu_project_fuses_paths_over_one_column(gpu_session, cpu_session,
                                                 gpu_calls):
    want = _fusion_frame(cpu_session).select(*_fusion_exprs("j")).to_pydict()
    assert gpu_calls == {"multi": 0, "single": 0}
    assert want["jn"] == [12, -7, None, None] and \
        want["jc"] == [5, -1, None, -1]
    q = _fusion_frame(gpu_session).select(*_fusion_exprs("j"))
    assert "GpuProject[get_json_object(" in q.explain()
    assert q.to_pydict() == want
    assert gpu_calls == {"multi": 1, "single": 0}

    gpu_calls.update(multi=0, single=0)
    off = sr.Session()
    off.set("spark.rapids.sql.enabled", True)
    off.set("spark.rapids.sql.json.combinePaths.enabled", False)
    q = _fusion_frame(off).select(*_fusion_exprs("j"))
    assert "GpuProject[get_json_object(" in q.explain()
    assert q.to_pydict() == want
    assert gpu_calls == {"multi": 0, "single": 4}


@pytest.mark.gpu
def test_gpu_project_fuses_each_json_column_apart(gpu_session, cpu_session,
                                                  gpu_calls):
    exprs = _fusion_exprs("j") + _fusion_exprs("j2")
    want = _fusion_frame(cpu_session).select(*exprs).to_pydict()
    got = _fusion_frame(gpu_session).select(*exprs).to_pydict()
    assert got == want
    assert gpu_calls == {"multi": 2, "single": 0}


@pytest.mark.gpu
def test_gpu_json_tuple(gpu_session, cpu_session, gpu_calls):
    rows = messy_corpus()
    fields = ["a", "b", "c", "s"]
    out = []
    for s in (cpu_session, gpu_session):
        df = s.create_dataframe({"j": rows}, dtypes={"j": DType.string()})
        s.register("tjt", df)
        q = df.select(sr.json_tuple(col("j"), *fields))
        if s is gpu_session:
            assert "GpuProject[json_tuple(" in q.explain(), q.explain()
        api = q.to_pydict()
        sql = s.sql("select json_tuple(j, 'a', 'b', 'c', 's') from tjt"
                    ).to_pydict()
        assert sql == api
        out.append(api)
    assert out[0] == out[1]
    assert sum(v is not None for v in out[0]["c0"]) > 50  # the fields hit
    # the DataFrame query and the SQL query: one batch, one parse each
    assert gpu_calls == {"multi": 2, "single": 0}
