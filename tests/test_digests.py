"""md5, sha1, sha2, crc32, hash and xxhash64.

The oracle is the standard library: every GPU result is compared with
hashlib / zlib of the bytes the test itself built, never with the CPU
backend. Every comparison is exact.

A STRING view whose offsets do not start at 0 is built by handing Column a
slice of another column's offsets over the same bytes.

In the end-to-end query `a` is a STRING column: concat_ws takes string
operands only.
"""
import hashlib
import os
import zlib

import numpy as np
import pytest
import torch

from spark_rapids_amd import (Column, DType, col, concat_ws, crc32, hash_,
                              lit, md5, sha1, sha2, xxhash64)
from spark_rapids_amd import ops
from spark_rapids_amd.column import make_validity
from spark_rapids_amd.expr import expressions as ex
from spark_rapids_amd.ops import cpu_backend
from spark_rapids_amd.plan.overrides import Tagger

I32, I64, F64, STR = (DType.int32(), DType.int64(), DType.float64(),
                      DType.string())
D128 = DType.decimal(30, 2)
ALGOS = ("md5", "sha1", "sha224", "sha256", "sha384", "sha512")
WIDTH = {"md5": 32, "sha1": 40, "sha224": 56, "sha256": 64, "sha384": 96,
         "sha512": 128}


def _frame(session, data, dtypes):
    return session.create_dataframe(data, dtypes=dtypes)


def _hex(algo, s):
    return None if s is None else hashlib.new(algo, s.encode()).hexdigest()


def _crc(s):
    return None if s is None else zlib.crc32(s.encode()) & 0xFFFFFFFF


def _text(k: int, salt: int = 0) -> str:
    """A string of exactly k UTF-8 bytes: the characters chr((7 * i + 131 *
    k + salt) & 0xFF), those above 0x7F as two bytes, the last one cut to
    ASCII where two bytes would not fit."""
    out = bytearray()
    i = 0
    while len(out) < k:
        b = (7 * i + 131 * k + salt) & 0xFF
        enc = chr(b).encode("utf-8")
        if len(out) + len(enc) > k:
            enc = bytes([b & 0x7F])
        out += enc
        i += 1
    s = out.decode("utf-8")
    assert len(s.encode("utf-8")) == k
    return s


# ---------------------------------------------------------------------------
# CPU backend, expressions, SQL, tagging, docs
# ---------------------------------------------------------------------------

def test_cpu_backend_known_answers():
    c = Column.from_pylist(["", "abc", None, "123456789"], STR)
    assert cpu_backend.digest_hex(c, "md5").to_pylist() == [
        "d41d8cd98f00b204e9800998ecf8427e",
        "900150983cd24fb0d6963f7d28e17f72", None,
        hashlib.md5(b"123456789").hexdigest()]
    assert cpu_backend.digest_hex(c, "sha1").to_pylist()[1] == \
        "a9993e364706816aba3e25717850c26c9cd0d89d"
    assert cpu_backend.digest_hex(c, "sha256").to_pylist()[1] == \
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    got = cpu_backend.crc32(c)
    assert got.dtype == I64
    assert got.to_pylist() == [0, zlib.crc32(b"abc"), None, 0xCBF43926]
    # the dispatchers reach the same functions
    assert ops.digest_hex(c, "sha512").to_pylist() == \
        [_hex("sha512", s) for s in c.to_pylist()]
    assert ops.crc32(c).to_pylist() == got.to_pylist()
    with pytest.raises(TypeError):
        cpu_backend.digest_hex(Column.from_pylist([1], I32), "md5")
    with pytest.raises(TypeError):
        cpu_backend.crc32(Column.from_pylist([1], I32))


def _six():
    return {"Md5": md5(col("s")), "Sha1": sha1(col("s")),
            "Sha2": sha2(col("s"), 256), "Crc32": crc32(col("s")),
            "Murmur3Hash": hash_(col("a"), col("s")),
            "XxHash64": xxhash64(col("a"), col("s"))}


DATA = {"a": [1, None, 3], "s": ["x", "yy", None], "d": [1.5, -0.0, None]}
DTS = {"a": I32, "s": STR, "d": F64}


def test_dtype_str_and_type_errors(cpu_session):
    sch = _frame(cpu_session, DATA, DTS).schema
    want = {"Md5": (STR, "md5(s)"), "Sha1": (STR, "sha1(s)"),
            "Sha2": (STR, "sha2(s, 256)"), "Crc32": (I64, "crc32(s)"),
            "Murmur3Hash": (I32, "hash(a, s)"),
            "XxHash64": (I64, "xxhash64(a, s)")}
    for name, e in _six().items():
        assert type(e).__name__ == name
        assert (e.dtype(sch), str(e)) == want[name], name
        assert all(isinstance(c, ex.Expression) for c in e.children)
    assert len(hash_(col("a"), col("s")).children) == 2
    for e in (md5(col("a")), sha1(col("d")), sha2(col("a"), 256),
              crc32(col("a")), md5(lit(1))):
        with pytest.raises(TypeError, match="needs a string input"):
            e.dtype(sch)
    # hash / xxhash64 take what the backends hash today and nothing else
    wide = _frame(cpu_session, {"m": [None], "l": [[1]]},
                  {"m": D128, "l": DType.list_(I32)}).schema
    for f in (hash_, xxhash64):
        for name in ("m", "l"):
            with pytest.raises(TypeError, match="not supported"):
                f(col(name)).dtype(wide)
        with pytest.raises(ValueError):
            f()
    for bits in (col("a"), "256", 2.0, None, True):
        with pytest.raises(ValueError, match="int literal"):
            sha2(col("s"), bits)
    assert sha2(col("s"), lit(512)).bits == 512


def test_cpu_results(cpu_session):
    df = _frame(cpu_session, DATA, DTS)
    got = df.select(md5(col("s")).alias("m"), sha1(col("s")).alias("s1"),
                    sha2(col("s"), 224).alias("s224"),
                    sha2(col("s"), 0).alias("s0"),
                    sha2(col("s"), 256).alias("s256"),
                    sha2(col("s"), 384).alias("s384"),
                    sha2(col("s"), 512).alias("s512"),
                    sha2(col("s"), 100).alias("bad"),
                    crc32(col("s")).alias("c")).to_pydict()
    s = DATA["s"]
    assert got["m"] == [_hex("md5", v) for v in s]
    assert got["s1"] == [_hex("sha1", v) for v in s]
    for bits in (224, 256, 384, 512):
        assert got[f"s{bits}"] == [_hex(f"sha{bits}", v) for v in s]
    assert got["s0"] == got["s256"]
    assert got["bad"] == [None, None, None]
    assert got["c"] == [_crc(v) for v in s]
    bad = sha2(col("s"), 100)
    assert bad.dtype(df.schema) == STR


def test_row_hashes_are_the_backend_functions(cpu_session):
    data = {"a": [1, None, -7, 2 ** 31 - 1], "d": [1.5, -0.0, None, 1e300],
            "s": ["x", None, "", "é" * 9]}
    dts = {"a": I32, "d": F64, "s": STR}
    df = _frame(cpu_session, data, dts)
    cols = [Column.from_pylist(data[k], dts[k]) for k in ("a", "d", "s")]
    got = df.select(hash_(col("a"), col("d"), col("s")).alias("h"),
                    xxhash64(col("a"), col("d"), col("s")).alias("x"),
                    hash_(col("s")).alias("h1")).to_pydict()
    assert got["h"] == cpu_backend.murmur3_hash(cols, 42).to_pylist()
    assert got["x"] == cpu_backend.xxhash64(cols, 42).to_pylist()
    assert got["h1"] == cpu_backend.murmur3_hash(cols[2:], 42).to_pylist()
    assert got["h1"][1] == 42  # a NULL operand leaves the seed
    assert None not in got["h"] + got["x"]
    # Spark's hash(1) and hash('x')
    one = _frame(cpu_session, {"a": [1]}, {"a": I32})
    assert one.select(hash_(col("a")).alias("h")).to_pydict()["h"] == \
        [-559580957]


def test_sql_spellings(cpu_session):
    cpu_session.register("t", _frame(cpu_session, DATA, DTS))

    def expr_of(text):
        plan = cpu_session.sql(f"SELECT {text} AS r FROM t")
        return plan.to_pydict()["r"], plan

    s = DATA["s"]
    assert expr_of("md5(s)")[0] == [_hex("md5", v) for v in s]
    assert expr_of("sha1(s)")[0] == expr_of("sha(s)")[0] == \
        [_hex("sha1", v) for v in s]
    assert expr_of("sha2(s, 512)")[0] == [_hex("sha512", v) for v in s]
    assert expr_of("sha2(s, 0)")[0] == [_hex("sha256", v) for v in s]
    assert expr_of("sha2(s, 7)")[0] == [None] * 3
    assert expr_of("crc32(s)")[0] == [_crc(v) for v in s]
    cols = [Column.from_pylist(DATA[k], DTS[k]) for k in ("a", "s")]
    assert expr_of("hash(a, s)")[0] == \
        cpu_backend.murmur3_hash(cols, 42).to_pylist()
    assert expr_of("xxhash64(a, s)")[0] == \
        cpu_backend.xxhash64(cols, 42).to_pylist()
    assert expr_of("md5(concat_ws('|', s, s))")[0] == \
        [_hex("md5", "|".join(p for p in (v, v) if p is not None))
         for v in s]


def test_sql_classes_and_argument_count(cpu_session):
    cpu_session.register("t", _frame(cpu_session, DATA, DTS))
    for text, cls in (("md5(s)", "Md5"), ("sha1(s)", "Sha1"),
                      ("sha(s)", "Sha1"), ("sha2(s, 256)", "Sha2"),
                      ("crc32(s)", "Crc32"), ("hash(a, s)", "Murmur3Hash"),
                      ("xxhash64(a)", "XxHash64")):
        text_plan = cpu_session.sql(f"SELECT {text} FROM t").explain()
        want = str(_six()[cls]) if text not in ("sha(s)", "xxhash64(a)") \
            else {"sha(s)": "sha1(s)", "xxhash64(a)": "xxhash64(a)"}[text]
        assert want in text_plan, (text, text_plan)
    for text in ("md5()", "md5(s, s)", "sha1()", "sha(s, s)", "sha2(s)",
                 "sha2(s, 256, 1)", "crc32()", "crc32(s, s)", "hash()",
                 "xxhash64()"):
        with pytest.raises(ValueError, match="takes"):
            cpu_session.sql(f"SELECT {text} FROM t")
    with pytest.raises(ValueError, match="int literal"):
        cpu_session.sql("SELECT sha2(s, a) FROM t")


def test_tagging(session):
    sch = _frame(session, DATA, DTS).schema
    t = Tagger(session.conf)
    for name, e in _six().items():
        assert t.expr_reasons(e, sch) == [], name
    assert t.expr_reasons(md5(concat_ws("|", col("s"), col("s"))), sch) == []
    assert t.expr_reasons(sha2(col("s"), 100), sch) == []
    for name, e in _six().items():
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
    rows = {ln.split("|")[1].strip(): [c.strip() for c in ln.split("|")]
            for ln in text.splitlines() if ln.startswith("| ")}
    for name in ("Md5", "Sha1", "Sha2", "Crc32", "Murmur3Hash", "XxHash64"):
        assert rows[name][3] == "GPU", (name, rows.get(name))
    assert "hash_(" in rows["Murmur3Hash"][4]
    assert "xxhash64(" in rows["XxHash64"][4]
    confs = open(os.path.join(str(tmp_path), "docs", "configs.md")).read()
    for name in ("Md5", "Sha1", "Sha2", "Crc32", "Murmur3Hash", "XxHash64"):
        assert f"`spark.rapids.sql.expression.{name}`" in confs
    # the committed documents are the generated ones
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for doc, new in (("supported_ops.md", text), ("configs.md", confs)):
        with open(os.path.join(repo, "docs", doc)) as f:
            assert f.read() == new, doc


# ---------------------------------------------------------------------------
# GPU: the kernels against hashlib / zlib
# ---------------------------------------------------------------------------

def _dev(values):
    return Column.from_pylist(values, STR).cuda()


def _check_all(values, column=None):
    """Every digest and crc32 of the column against the standard library;
    returns the result columns by algorithm."""
    c = _dev(values) if column is None else column
    out = {}
    for algo in ALGOS:
        r = ops.digest_hex(c, algo)
        assert r.dtype == STR and r.size == len(values)
        w = WIDTH[algo]
        offs = r.offsets.cpu().numpy()
        assert r.offsets.dtype == torch.int32
        assert (offs == np.arange(len(values) + 1, dtype=np.int64) * w).all()
        assert r.data.numel() == len(values) * w
        got = r.to_pylist()
        want = [_hex(algo, v) for v in values]
        bad = [i for i in range(len(values)) if got[i] != want[i]]
        assert not bad, (algo, bad[:5], got[bad[0]], want[bad[0]])
        out[algo] = r
    r = ops.crc32(c)
    assert r.dtype == I64
    got, want = r.to_pylist(), [_crc(v) for v in values]
    bad = [i for i in range(len(values)) if got[i] != want[i]]
    assert not bad, ("crc32", bad[:5], got[bad[0]], want[bad[0]])
    out["crc32"] = r
    return out


@pytest.fixture(scope="module")
def every_length():
    return [_text(k) for k in range(261)]


@pytest.mark.gpu
def test_gpu_every_boundary(every_length):
    """Row k has k bytes: every pad boundary of both block sizes, one to
    three blocks, and (the rows being consecutive) every start alignment."""
    starts = np.cumsum([0] + [len(s.encode()) for s in every_length])
    assert {int(x) % 16 for x in starts} == set(range(16))
    assert any(ord(ch) > 0x7F for s in every_length for ch in s)
    _check_all(every_length)


@pytest.mark.gpu
def test_gpu_grid_shape_and_nulls():
    rng = np.random.default_rng(18)
    values = [None if rng.random() < 0.1 else
              _text(int(rng.integers(0, 201)), int(rng.integers(0, 256)))
              for _ in range(1000)]
    for i in (0, 63, 64, 255, 256, 999):
        values[i] = None
    out = _check_all(values)
    nulls = sum(v is None for v in values)
    for algo, r in out.items():
        assert r.null_count == nulls, algo
    # a null row's bytes are '0' digits, not whatever the allocation held
    r = out["sha1"]
    raw = r.data.cpu().numpy().reshape(1000, 40)
    for i in (0, 63, 64, 255, 256, 999):
        assert bytes(raw[i]) == b"0" * 40
    assert out["crc32"].data.cpu().numpy()[[0, 63, 64, 255, 256, 999]] \
        .tolist() == [0] * 6


@pytest.mark.gpu
def test_gpu_degenerate_inputs():
    for algo in ALGOS:
        r = ops.digest_hex(_dev([]), algo)
        assert r.size == 0 and r.dtype == STR and r.to_pylist() == []
    r = ops.crc32(_dev([]))
    assert r.size == 0 and r.dtype == I64
    out = _check_all([None] * 130)
    assert all(r.null_count == 130 for r in out.values())
    _check_all([""])
    _check_all(["", "", None, ""])
    with pytest.raises(TypeError):
        ops.digest_hex(Column.from_pylist([1], I32).cuda(), "md5")
    with pytest.raises(TypeError):
        ops.crc32(Column.from_pylist([1], I32).cuda())


@pytest.mark.gpu
def test_gpu_view_with_offsets_not_at_zero(every_length):
    base = _dev(every_length)
    lo, hi = 37, 201
    valid = np.ones(hi - lo, dtype=bool)
    valid[[0, 5, 64]] = False
    view = Column(STR, hi - lo, base.data, make_validity(valid, "cuda"),
                  base.offsets[lo:hi + 1])
    assert int(view.offsets[0]) != 0
    values = [v if ok else None
              for v, ok in zip(every_length[lo:hi], valid)]
    _check_all(values, view)
    # and equals its materialised copy
    copy = _dev(values)
    assert ops.digest_hex(view, "sha384").to_pylist() == \
        ops.digest_hex(copy, "sha384").to_pylist()


@pytest.mark.gpu
def test_gpu_two_long_rows_among_short_ones():
    values = [_text(k % 23, k) for k in range(150)]
    values[5] = _text(1000, 3)
    values[77] = _text(4097, 9)
    _check_all(values)


@pytest.mark.gpu
def test_gpu_result_over_int32_offsets_raises():
    n = 2 ** 31 // 128
    c = Column(STR, n, torch.zeros(0, dtype=torch.uint8, device="cuda"), None,
               torch.zeros(n + 1, dtype=torch.int32, device="cuda"), 0)
    with pytest.raises(OverflowError,
                       match="sha512 result exceeds int32 offsets"):
        ops.digest_hex(c, "sha512")


E2E_SQL = ("SELECT md5(concat_ws('|', a, s)), sha2(s, 256), sha2(s, 512), "
           "sha1(s), crc32(s), hash(a, s), xxhash64(a, s) FROM t")


def _e2e_data():
    rng = np.random.default_rng(7)
    a = [None if rng.random() < 0.1 else f"k{int(rng.integers(0, 50))}"
         for _ in range(300)]
    s = [None if rng.random() < 0.15 else
         _text(int(rng.integers(0, 140)), int(rng.integers(0, 256)))
         for _ in range(300)]
    return {"a": a, "s": s}


def _e2e_exprs():
    return [md5(concat_ws("|", col("a"), col("s"))), sha2(col("s"), 256),
            sha2(col("s"), 512), sha1(col("s")), crc32(col("s")),
            hash_(col("a"), col("s")), xxhash64(col("a"), col("s"))]


@pytest.mark.gpu
def test_gpu_and_cpu_sessions_agree_end_to_end(gpu_session, cpu_session):
    data = _e2e_data()
    dts = {"a": STR, "s": STR}
    out = []
    for sess in (gpu_session, cpu_session):
        df = _frame(sess, data, dts)
        sess.register("t", df)
        by_api = df.select(*[e.alias(f"c{i}")
                             for i, e in enumerate(_e2e_exprs())])
        by_sql = sess.sql(E2E_SQL)
        if sess is gpu_session:
            for plan in (by_api, by_sql):
                tree = plan.physical_plan().tree_string()
                assert "GpuProject" in tree and "cpu_bridge" not in tree \
                    and "CpuProject" not in tree, tree
        out.append([list(by_api.to_pydict().values()),
                    list(by_sql.to_pydict().values())])
    assert out[0][0] == out[0][1] == out[1][0] == out[1][1]
    a, s = data["a"], data["s"]
    got = out[0][0]
    assert got[0] == [_hex("md5", "|".join(p for p in r if p is not None))
                      for r in zip(a, s)]
    assert got[1] == [_hex("sha256", v) for v in s]
    assert got[2] == [_hex("sha512", v) for v in s]
    assert got[3] == [_hex("sha1", v) for v in s]
    assert got[4] == [_crc(v) for v in s]
    assert None not in got[5] + got[6]
