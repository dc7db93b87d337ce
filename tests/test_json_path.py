"""get_json_object over nested paths, array indexes and escaped strings:
the path parser, the host semantics, the device row parser run on the host
(native/hipdf/tests/json_path_host_test.cpp) and, on the GPU, the kernel
against the CPU backend with an account of which rows went to the host."""
import os
import random
import shutil
import subprocess

import pytest

import spark_rapids_amd as sr
from spark_rapids_amd import Column, DType, col
from spark_rapids_amd.expr import json_path
from spark_rapids_amd.expr.expressions import GetJsonObject
from spark_rapids_amd.expr.json_path import INDEX, KEY
from spark_rapids_amd.ops import cpu_backend

U = chr(92) + "u"  # spelt out so that no tool rewrites the escapes below
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "native", "hipdf")

P16 = "$" + ".a" * 16
P17 = "$" + ".a" * 17
PATHS = ["$", "$.a", "$.a.b", "$.a[1]", "$.a[1].b", "$['k k']", "$.s",
         "$.missing", "$.a[99]", P16, P17]
GEN_PATHS = ["$", "$.a", "$.a.b", "$.a[1]", "$.a[1].b", "$.s", "$.b.c[0]",
             "$[0].a"]


def _nest(depth, leaf="7"):
    return '{"a":' * depth + leaf + "}" * depth


# every document is written out: the expectations come from the CPU backend
HAND = [
    # plain shapes the paths hit
    '{"a":1}',
    '{"a":{"b":1}}',
    '{"a":[10,{"b":"x"}],"c d":{"e":null}}',
    '{"a":[1,2,3]}',
    '{"a":[{"b":1},{"b":2}]}',
    '{"k k":"v","s":"str"}',
    '{"s":"plain","k k":{"x":[1,2]}}',
    '{"a":[[1,2],[3,4]]}',
    '{"a":{"1":2}}',
    '[{"a":1}]',
    '[0,[1,{"b":2}]]',
    _nest(16),
    _nest(17),
    _nest(18, '"deep"'),
    # every escape, \u forms and a surrogate pair as a string result
    r'{"s":"q\"q"}',
    r'{"s":"b\\b"}',
    r'{"s":"sl\/ash"}',
    r'{"s":"\b\f\n\r\t"}',
    '{"s":"' + U + "0041" + U + "00e9" + U + '20ac"}',
    '{"s":"' + U + "00e9" + U + '00C9"}',
    '{"s":"' + U + "d83d" + U + 'de00 ok"}',
    '{"s":"x' + U + "d834" + U + 'dd1ey","a":"' + U + "d83d" + U + 'de00"}',
    '{"s":"été €","a":{"b":"é"}}',
    # escapes and non-ascii inside an object / array result
    r'{"a":{"b":"x\ny"}}',
    r'{"a":["t\tt",{"b":"q\"q"}]}',
    '{"a":{"é":1}}',
    # escaped keys on and off the path
    '{"' + U + '0061":1}',
    r'{"a\\":1,"a":2}',
    '{"a":3,"z":{"' + U + '0061":1}}',
    '{"' + U + '0061":{"b":5,"c":6}}',
    # numbers
    '{"a":-12,"s":1.25}',
    '{"a":0,"s":-0.5}',
    '{"a":1e2}',
    '{"a":12.50}',
    '{"a":0.00001}',
    '{"a":0.0001}',
    '{"a":-0}',
    '{"a":-0.0}',
    '{"a":1E5,"s":2}',
    '{"a":[1.0,2.5e3]}',
    '{"a":[1.5,-3,0.25]}',
    '{"a":123456789012345678901234567890}',
    '{"a":1234567890.1234567}',
    '{"a":123456789.123456}',
    '{"s":7,"a":{"b":1e2}}',
    # literals
    '{"a":true,"s":false}',
    '{"a":null,"s":null}',
    '{"a":[null,null]}',
    '{"a":NaN}',
    '{"a":[Infinity,-Infinity]}',
    '{"s":"x","zz":NaN}',
    # root scalars
    '5', '"str"', 'true', 'null', '-0', '1.5', ' [1,2] ',
    # whitespace of all four kinds in every position
    ' \t\n\r{ \t"a" \n: \r[ 1 ,\t{ "b" : "x" } \n] , "s" : " keep  this " } \n',
    '{"a": { "b" : [ 1 , 2 ] , "c" : "x y" } }',
    '\n[\n1\n,\n2\n]\n',
    # empty containers and the empty key
    '{}', '[]', '{"a":{}}', '{"a":[]}', '{"a":[[],{}]}',
    '{"":1,"a":{"":2}}',
    # depth is part of the match
    '{"x":{"a":1},"a":2}',
    '{"x":{"s":1},"y":[{"s":2}],"s":3}',
    # a key that occurs inside a string value
    '{"x":"{a:1, s:2}","a":4,"s":"a"}',
    r'{"x":"\"a\":5","a":6,"s":"\"s\":1"}',
    '{"a":{"b":"}{][,:  "}}',
    # invalid documents, one per class
    '{"a":1', '{"a":1}}', '{"a":1} x', '{"a" 1}', '{a:1}', '{"a":1,}',
    '[1,]', '{"a":[1,2}', '{"a":"unterminated}', '{"s":"a\tb"}',
    r'{"s":"\x"}', r'{"s":"\u12"}', r'{"s":"\u12G4"}', '{"a":01}',
    '{"a":1.}', '{"a":.5}', '{"a":+1}', '{"a":1e}', '{"a":-}', '{"a":1e+}',
    '{"a":tru}', '{"a":nul}', '{"a":True}', '{"a":falsee}', '{"a":-NaN}',
    '{"a":1 "s":2}', '{,"a":1}', '[}', '{"a"}', '{"a":}', ',',
    '{"a":1}{"a":2}', '{"a":2,"s":"x"]', '{"a":[1,{"b":"x"}],"s":1',
    # NULL, empty and blank rows
    None, '', ' \t\n\r',
    # a long document
    '{"pad":"' + "x" * 4950 + '","a":[1,{"b":"deep"}],"s":"end"}',
    # nesting depth exactly 64 and 65
    "[" * 64 + "]" * 64,
    "[" * 65 + "]" * 65,
    '{"a":' + "[" * 63 + "1" + "]" * 63 + "}",
    '{"a":' + "[" * 64 + "1" + "]" * 64 + "}",
]


# Duplicated keys on the path: the last wins. Each document goes with the
# paths whose result does not itself contain the duplicated member: there the
# device copies both members where the host's dict keeps one, the documented
# divergence.
DUPS = [
    ('{"a":1,"a":2}', ("$.a", "$.a.b", "$.s")),
    ('{"a":{"b":1},"a":{"c":2}}', ("$.a", "$.a.b", "$.a[1]")),
    ('{"a":{"b":1},"a":{"b":3}}', ("$.a", "$.a.b")),
    ('{"a":{"b":{"c":1}},"a":{"b":3},"s":{"b":4}}', ("$.a", "$.a.b", "$.s")),
    ('{"a":1,"a":null}', ("$.a",)),
    ('{"a":null,"a":[1,2]}', ("$.a", "$.a[1]")),
    ('{"a":[0,{"b":1,"b":2}]}', ("$.a[1].b", "$.a.b", "$.s")),
    ('{"a":1e2,"a":3}', ("$.a",)),
    ('{"a":3,"a":1e2}', ("$.a",)),
    ('{"a":[10,20],"a":[30,{"b":"y"}]}', ("$.a", "$.a[1]", "$.a[1].b")),
    ('{"s":"x","a":[5,{"b":1}],"s":"y","a":[6]}', ("$.a", "$.a[1]", "$.s")),
]


def _cpu_answers(rows, path):
    return cpu_backend.get_json_object(
        Column.from_pylist(rows, DType.string()), path).to_pylist()


# ---- generated corpora ------------------------------------------------------

_WS = [" ", "\t", "\n", "\r"]


def _ws(rng):
    return "".join(rng.choice(_WS) for _ in range(rng.choice((0, 0, 0, 1, 2))))


def _canonical_float(rng):
    ip = str(rng.randrange(0, 100000))
    if rng.random() < 0.2:
        frac = "0"
    else:  # may start with zeros, never ends in one
        frac = "".join(rng.choice("0123456789")
                       for _ in range(rng.randrange(0, 4))) + rng.choice(
                           "123456789")
    return ("-" if rng.random() < 0.3 else "") + ip + "." + frac


def _clean_scalar(rng):
    k = rng.randrange(6)
    if k == 0:
        v = rng.randrange(-10 ** 6, 10 ** 6)
        return str(v)
    if k == 1:
        return _canonical_float(rng)
    if k == 2:
        n = rng.randrange(0, 9)
        return '"' + "".join(rng.choice("abcxyz {}[],:019")
                             for _ in range(n)) + '"'
    return ("true", "false", "null")[k - 3]


def _messy_scalar(rng):
    k = rng.randrange(8)
    if k == 0:
        return rng.choice(["1e2", "12.50", "0.00001", "-0", "1E-3", "2.5e+7",
                           "0.10", "100.0", "-0.0", "1234567.12345678901",
                           "3.0e0", "17", "-4.25"])
    if k == 1:
        parts = [rng.choice([r"\"", r"\\", r"\/", r"\b", r"\f", r"\n", r"\r",
                             r"\t", U + "0041", U + "00e9",
                             U + "20ac", U + "d83d" + U + "de00", "é",
                             "中", "ab", " "])
                 for _ in range(rng.randrange(0, 5))]
        return '"' + "".join(parts) + '"'
    return _clean_scalar(rng)


def _gen_value(rng, depth, scalar):
    if depth >= 5 or rng.random() < 0.35:
        return scalar(rng)
    return _gen_container(rng, depth, scalar)


def _gen_container(rng, depth, scalar):
    n = rng.randrange(0, 4)
    if rng.random() < 0.6:
        items = []
        # distinct keys: an object result with a duplicated key is the one
        # documented divergence (the device copies both members)
        for key in rng.sample(["a", "b", "c", "s"], n):
            items.append(_ws(rng) + '"' + key + '"' + _ws(rng) + ":" +
                         _ws(rng) + _gen_value(rng, depth + 1, scalar) +
                         _ws(rng))
        return "{" + (",".join(items) if items else _ws(rng)) + "}"
    items = [_ws(rng) + _gen_value(rng, depth + 1, scalar) + _ws(rng)
             for _ in range(n)]
    return "[" + (",".join(items) if items else _ws(rng)) + "]"


def _damage(rng, doc):
    """Delete or duplicate one structural character, or truncate. A comma
    between two digits is left alone: without it `1.5,10` would read as the
    float `1.510`, a text the device hands to the host, and this corpus is
    the one on which the host must not be asked at all."""
    k = rng.randrange(3)
    if k == 2:
        return doc[:rng.randrange(0, len(doc))]
    spots = [i for i, c in enumerate(doc) if c in '{}[],:"'
             and not (c == "," and k == 0 and 0 < i < len(doc) - 1
                      and doc[i - 1].isdigit() and doc[i + 1].isdigit())]
    i = rng.choice(spots)
    return doc[:i] + doc[i + 1:] if k == 0 else doc[:i] + doc[i] + doc[i:]


def clean_corpus(n=2000, seed=20):
    rng = random.Random(seed)
    rows = []
    for _ in range(n):
        doc = _ws(rng) + _gen_container(rng, 1, _clean_scalar) + _ws(rng)
        if rng.random() < 0.25:
            doc = _damage(rng, doc)
        rows.append(doc)
    return rows


def messy_corpus(n=500, seed=21):
    rng = random.Random(seed)
    return [_ws(rng) + _gen_container(rng, 1, _messy_scalar) + _ws(rng)
            for _ in range(n)]


# ---- path parser ------------------------------------------------------------

def test_parse_grammar():
    assert json_path.parse("$") == []
    assert json_path.parse("$.a") == [(KEY, "a")]
    assert json_path.parse("$['a']") == [(KEY, "a")]
    assert json_path.parse("$['c d']['']") == [(KEY, "c d"), (KEY, "")]
    assert json_path.parse("$['x]y.z']") == [(KEY, "x]y.z")]
    assert json_path.parse("$[0]") == [(INDEX, 0)]
    assert json_path.parse("$.a[12].b['c'][0][1]") == [
        (KEY, "a"), (INDEX, 12), (KEY, "b"), (KEY, "c"), (INDEX, 0),
        (INDEX, 1)]
    assert json_path.parse("$[007]") == [(INDEX, 7)]
    assert json_path.parse("$.a b[1]") == [(KEY, "a b"), (INDEX, 1)]


def test_parse_legacy_equivalence():
    for p in ("$.k", "$.a.b", "$", "$.", "$..a", "$a.b", "$.a.", "$.a b.c"):
        legacy = [k for k in p[1:].lstrip(".").split(".") if k]
        assert json_path.parse(p) == [(KEY, k) for k in legacy], p


def test_parse_malformed_is_none():
    for p in ("$.a[", "$[x]", "$.a[1", "$[1]x", "$['a'", "$['a]", "$[]",
              "$.a[-1]", "$.[0]", "$[0]..a", "$[0].", "$['a']b", "a.b", "",
              "$[1.5]", "$[ 1]"):
        assert json_path.parse(p) is None, p


def test_wildcards_raise_at_construction():
    for p in ("$.a[*]", "$.*", "$[*]", "$.a.*", "$[0].*"):
        with pytest.raises(NotImplementedError, match="json path wildcard"):
            GetJsonObject(col("j"), p)


def test_encode():
    flat, names = json_path.encode([(KEY, "ab"), (INDEX, 3), (KEY, ""),
                                    (KEY, "é"), (INDEX, 2 ** 40)])
    assert flat == [0, 0, 2, 1, 3, 0, 0, 2, 0, 0, 2, 2, 1, 2 ** 31 - 1, 0]
    assert names == b"ab\xc3\xa9"


# ---- host semantics ---------------------------------------------------------

def _host(doc, path):
    s = sr.Session({"spark.rapids.sql.enabled": False})
    df = s.create_dataframe({"j": [doc]})
    return df.select(col("j").get_json_object(path).alias("r")
                     ).to_pydict()["r"][0]


def test_host_nested_paths():
    doc = '{"a":[10,{"b":"x"}],"c d":{"e":null}}'
    assert _host(doc, "$.a[1].b") == "x"
    assert _host(doc, "$.a[0]") == "10"
    assert _host(doc, "$.a[2]") is None
    assert _host(doc, "$['c d']") == '{"e":null}'
    assert _host(doc, "$.a") == '[10,{"b":"x"}]'
    assert _host(doc, "$['c d'].e") is None
    assert _host('{"a":[1]}', "$.a.b") is None
    assert _host('{"a":{"0":1}}', "$.a[0]") is None
    assert _host('{"a":1,"a":2}', "$.a") == "2"
    assert _host('{"a":{"b":1},"a":{"c":2}}', "$.a.b") is None


def test_host_malformed_path_is_all_null(cpu_session):
    df = cpu_session.create_dataframe({"j": ['{"a":[1]}', None, "x"]})
    out = df.select(col("j").get_json_object("$.a[").alias("r")).to_pydict()
    assert out["r"] == [None, None, None]


def test_host_sql_matches_dataframe(cpu_session):
    df = cpu_session.create_dataframe(
        {"j": ['{"a":[10,{"b":"x"}]}', '{"a":[1]}', None]})
    cpu_session.register("tj", df)
    got = cpu_session.sql(
        "select get_json_object(j, '$.a[1].b') from tj").collect()
    assert got == [("x",), (None,), (None,)]


def test_tagger_bounds_path_length(session):
    from spark_rapids_amd.plan.overrides import Tagger

    schema = session.create_dataframe({"j": ["{}"]}).schema
    t = Tagger(session.conf)
    assert t.expr_reasons(GetJsonObject(col("j"), "$.a[1].b"), schema) == []
    assert t.expr_reasons(GetJsonObject(col("j"), P16), schema) == []
    assert t.expr_reasons(GetJsonObject(col("j"), P17), schema) == \
        ["json paths of more than 16 steps run on CPU"]


# ---- the device parser, run on the host ------------------------------------

def _hex(s):
    return "x" + s.encode("utf-8").hex()


def _write_cases(path, steps, rows, answers):
    with open(path, "w") as f:
        f.write(f"{len(steps)}\n")
        for kind, arg in steps:
            f.write(f"k {_hex(arg)}\n" if kind == KEY else f"i {arg}\n")
        for doc, want in zip(rows, answers):
            f.write(f"{_hex(doc)} {'-' if want is None else _hex(want)}\n")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("jp") / "json_path_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall",
                    "-I" + os.path.join(NATIVE, "kernels"),
                    os.path.join(NATIVE, "tests", "json_path_host_test.cpp"),
                    "-o", exe], check=True)
    return exe


def test_row_parser_on_host_matches_host_backend(host_exe, tmp_path):
    exe = host_exe
    common = [r for r in HAND if r is not None] + clean_corpus() + \
        messy_corpus()
    for i, p in enumerate(dict.fromkeys(PATHS + GEN_PATHS)):
        rows = common + [doc for doc, paths in DUPS if p in paths]
        cases = str(tmp_path / f"cases{i}.txt")
        _write_cases(cases, json_path.parse(p), rows, _cpu_answers(rows, p))
        run = subprocess.run([exe, cases], capture_output=True, text=True)
        print(p, run.stdout[-400:])
        assert run.returncode == 0, (p, run.stdout[-2000:], run.stderr)


def test_row_parser_flags_lone_surrogates(host_exe, tmp_path):
    # the host backend cannot put a lone surrogate into a column, so these
    # rows have no recorded answer: the parser must leave every one to the
    # host, and must still answer the paired form itself
    lone = ['{"s":"' + U + 'd83d"}', '{"s":"' + U + 'de00x"}',
            '{"s":"' + U + "d83d" + U + '0041"}',
            '{"s":"' + U + "d83d" + U + "d83d" + U + 'de00"}',
            '{"s":"x' + U + 'd83d\\n"}']
    cases = str(tmp_path / "lone.txt")
    _write_cases(cases, json_path.parse("$.s"), lone, [None] * len(lone))
    run = subprocess.run([host_exe, cases], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout
    assert f"flagged {len(lone)} " in run.stdout, run.stdout
    pair = ['{"s":"' + U + "d83d" + U + 'de00"}']
    _write_cases(cases, json_path.parse("$.s"), pair, ["\U0001F600"])
    run = subprocess.run([host_exe, cases], capture_output=True, text=True)
    assert run.returncode == 0 and "flagged 0 " in run.stdout, run.stdout


# ---- GPU --------------------------------------------------------------------

def _select_all(session, rows, paths):
    df = session.create_dataframe({"j": rows}, dtypes={"j": DType.string()})
    return df.select(*[col("j").get_json_object(p).alias(f"p{i}")
                       for i, p in enumerate(paths)]).to_pydict()


@pytest.fixture
def host_calls(monkeypatch):
    """Sizes of the columns the GPU backend hands to the host backend."""
    calls = []
    real = cpu_backend.get_json_object

    def recording(c, path):
        calls.append(c.size)
        return real(c, path)

    def arm():
        monkeypatch.setattr(cpu_backend, "get_json_object", recording)
        return calls

    return arm


@pytest.mark.gpu
def test_gpu_hand_corpus(gpu_session, cpu_session):
    rows = (HAND * 3)[:193]  # three waves plus one lane
    assert len(rows) == 193 and len(HAND) <= 193
    want = _select_all(cpu_session, rows, PATHS)
    got = _select_all(gpu_session, rows, PATHS)
    for i, p in enumerate(PATHS):
        for r, (g, w) in enumerate(zip(got[f"p{i}"], want[f"p{i}"])):
            assert g == w, (p, rows[r], g, w)


@pytest.mark.gpu
def test_gpu_literal_answers(gpu_session):
    rows = ['{"x":{"a":1},"a":2}', '{"a":1', '{"a":{"b":1},"a":{"c":2}}',
            '{"a":"' + U + "d83d" + U + 'de00\\n"}', '{"a":[10,{"b":"x"}]}']
    got = _select_all(gpu_session, rows, ["$.a", "$.a.b", "$.a[1].b"])
    assert got["p0"] == ["2", None, '{"c":2}', "\U0001F600\n",
                         '[10,{"b":"x"}]']
    assert got["p1"] == [None] * 5
    assert got["p2"] == [None, None, None, None, "x"]


@pytest.mark.gpu
def test_gpu_duplicated_keys_last_wins(gpu_session, cpu_session):
    rows = [doc for doc, _ in DUPS]
    paths = sorted({p for _, ps in DUPS for p in ps})
    want = _select_all(cpu_session, rows, paths)
    got = _select_all(gpu_session, rows, paths)
    for i, p in enumerate(paths):
        for (doc, ps), g, w in zip(DUPS, got[f"p{i}"], want[f"p{i}"]):
            if p in ps:
                assert g == w, (p, doc, g, w)
    assert want[f"p{paths.index('$.a.b')}"][1] is None
    assert want[f"p{paths.index('$.a')}"][0] == "2"


@pytest.mark.gpu
def test_gpu_single_row(gpu_session, cpu_session):
    rows = ['{"a":[10,{"b":"x"}],"s":"q\\"q"}']
    assert _select_all(gpu_session, rows, PATHS) == \
        _select_all(cpu_session, rows, PATHS)


@pytest.mark.gpu
def test_gpu_plan_placement(gpu_session):
    df = gpu_session.create_dataframe({"j": ['{"a":1}']})
    text = df.select(col("j").get_json_object(P16).alias("r")).explain()
    assert "GpuProject[get_json_object(" in text, text
    text = df.select(col("j").get_json_object(P17).alias("r")).explain()
    assert "CpuProject[get_json_object(" in text, text
    assert "json paths of more than 16 steps run on CPU" in text, text


@pytest.mark.gpu
def test_gpu_column_slice_with_nonzero_first_offset():
    from spark_rapids_amd.ops import gpu_backend

    rows = [r for r in HAND if r is not None][:60]
    full = Column.from_pylist(rows, DType.string()).cuda()
    k = 7
    part = Column(DType.string(), full.size - k, full.data, None,
                  full.offsets[k:], 0)
    assert int(part.offsets[0].item()) > 0
    for p in ("$.a", "$.a[1].b", "$.s", "$"):
        got = gpu_backend.get_json_object(part, p).to_pylist()
        assert got == _cpu_answers(rows[k:], p), p


@pytest.mark.gpu
def test_gpu_malformed_path_is_all_null(gpu_session):
    got = _select_all(gpu_session, ['{"a":[1]}', None, "x"], ["$.a["])
    assert got["p0"] == [None, None, None]


FLAGGED = [
    '{"a":1e2}',                 # a non-canonical float is the result
    '{"a":[12.50]}',             # ... inside an array result
    '{"a":{"t":"é"}}',      # non-ascii inside an object result
    '{"a":1,"z":NaN}',           # a Python-only literal anywhere
    '{"' + U + '0061":1}',      # an escaped key where $.a is matched
]
UNFLAGGED = [                    # the same constructs off the path
    '{"a":1,"z":1e2}',
    '{"a":[1],"z":[12.50]}',
    '{"a":{"t":"e"},"z":{"t":"é"}}',
    '{"a":2,"z":{"' + U + '0061":1}}',
    '{"a":"é"}',
    r'{"a":"x\nyé"}',
    '{"a":{"n":[1.5,-3]},"z":-0}',
]


@pytest.mark.gpu
def test_gpu_flagged_rows_only_go_to_host(gpu_session, cpu_session,
                                          host_calls):
    rows = [None] * 12
    rows[0::5] = FLAGGED[:3]          # rows 0, 5, 10
    rows[3], rows[7] = FLAGGED[3:]
    rest = iter(UNFLAGGED)
    rows = [r if r is not None else next(rest) for r in rows]
    assert len(rows) == 12
    want = _select_all(cpu_session, rows, ["$.a"])
    calls = host_calls()
    got = _select_all(gpu_session, rows, ["$.a"])
    assert calls == [5], calls
    assert got == want
    assert want["p0"][0] == "100.0" and want["p0"][5] == "[12.5]"


@pytest.mark.gpu
def test_gpu_clean_corpus_never_asks_host(gpu_session, cpu_session,
                                          host_calls):
    rows = clean_corpus()
    want = _select_all(cpu_session, rows, GEN_PATHS)
    assert sum(v is not None for v in want["p1"]) > 200  # the paths hit
    calls = host_calls()
    got = _select_all(gpu_session, rows, GEN_PATHS)
    assert calls == [], calls
    for i, p in enumerate(GEN_PATHS):
        for r, (g, w) in enumerate(zip(got[f"p{i}"], want[f"p{i}"])):
            assert g == w, (p, rows[r], g, w)


@pytest.mark.gpu
def test_gpu_hand_corpus_without_flags_never_asks_host(gpu_session,
                                                       cpu_session,
                                                       host_calls):
    rows = HAND[:14] + ['{"a":1', None, "", '{"x":{"a":1},"a":2}']
    want = _select_all(cpu_session, rows, PATHS[:9])
    calls = host_calls()
    got = _select_all(gpu_session, rows, PATHS[:9])
    assert calls == [], calls
    assert got == want


@pytest.mark.gpu
def test_gpu_messy_corpus(gpu_session, cpu_session):
    rows = messy_corpus()
    want = _select_all(cpu_session, rows, GEN_PATHS)
    got = _select_all(gpu_session, rows, GEN_PATHS)
    for i, p in enumerate(GEN_PATHS):
        for r, (g, w) in enumerate(zip(got[f"p{i}"], want[f"p{i}"])):
            assert g == w, (p, rows[r], g, w)


@pytest.mark.gpu
def test_gpu_sql_matches_dataframe(gpu_session, cpu_session):
    rows = [r for r in HAND if r is not None][:40]
    out = []
    for s in (gpu_session, cpu_session):
        df = s.create_dataframe({"j": rows})
        s.register("tjson", df)
        sql = s.sql("select get_json_object(j, '$.a[1].b') from tjson"
                    ).collect()
        api = df.select(col("j").get_json_object("$.a[1].b")).collect()
        assert sql == api
        out.append(sql)
    assert out[0] == out[1]
    assert ("x",) in out[0]
