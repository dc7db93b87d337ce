"""array_position / array_remove / slice over LIST<int64> next to the lambda
spelling of the same work: (a) array_position(a, v) against
exists(a, x -> x = v), (b) array_remove(a, v) against filter(a, x -> x != v),
(c) slice(a, s, n) against filter(a, (x, i) -> i >= s0 and i < e) with
s0 = s - 1 and e = s0 + n ready as columns. v is taken from its row in about
half the rows and is absent from the others. array_repeat(v, c) has no other
spelling and is timed alone. Expressions are evaluated on a device batch
directly; each pair is first checked to agree, then one warm-up and 5 repeats
alternating candidate and baseline inside one process, host clock around a
device synchronise.
Usage: python tools/bench_list_search.py [out.json]
(results recorded in profiles/r12_array_search.md)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_amd import (Column, ColumnBatch, DType, Field,  # noqa: E402
                              Schema, array_repeat, col)
from spark_rapids_amd.ops import gpu_backend as g  # noqa: E402

I32, I64 = DType.int32(), DType.int64()
L_I64 = DType.list_(I64)


def _fixed(arr, dt):
    return Column(dt, len(arr), torch.from_numpy(arr).cuda(), None,
                  null_count=0)


def make(nrows, lo, hi, seed):
    """(device batch [a, v, s, n, s0, e, c], schema)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, nrows).astype(np.int64)
    offs = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[-1])
    vals = rng.integers(0, 1 << 40, total, dtype=np.int64)
    # the needle: an element of the row for about half the rows, -1 else
    pick = offs[:-1] + (rng.random(nrows) * lens).astype(np.int64)
    take = (rng.random(nrows) < 0.5) & (lens > 0)
    v = np.where(take, vals[np.minimum(pick, max(total - 1, 0))], -1)
    s = (1 + rng.integers(0, max(lo, 3), nrows)).astype(np.int32)
    n = np.full(nrows, max((lo + hi) // 4, 1), dtype=np.int32)
    a = Column(L_I64, nrows, torch.zeros(0, dtype=torch.uint8, device="cuda"),
               None, torch.from_numpy(offs.astype(np.int32)).cuda(), 0,
               _fixed(vals, I64))
    c = rng.integers(0, 9, nrows).astype(np.int32)
    cols = [a, _fixed(v, I64), _fixed(s, I32), _fixed(n, I32),
            _fixed(s - 1, I32), _fixed(s - 1 + n, I32), _fixed(c, I32)]
    schema = Schema([Field("a", L_I64), Field("v", I64), Field("s", I32),
                     Field("n", I32), Field("s0", I32), Field("e", I32),
                     Field("c", I32)])
    return ColumnBatch(cols, nrows), schema


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _same_lists(x, y):
    return x.child.size == y.child.size and \
        bool(torch.equal(x.offsets, y.offsets)) and \
        bool(torch.equal(x.child.data, y.child.data))


def main():
    res = {}
    for name, nrows, lo, hi in (("short_4M_len0-8", 4_000_000, 0, 8),
                                ("block_64K_len900-1100", 65_536, 900, 1100)):
        batch, schema = make(nrows, lo, hi, 1)
        a = batch.columns[0]
        mean_len = -(-a.child.size // nrows)
        entry = {"rows": nrows, "elements": a.child.size,
                 "find_width": g._list_group_width(mean_len)}
        arr, v = col("a"), col("v")
        cases = {
            "array_position": (
                arr.array_position(v), arr.exists(lambda x: x == v)),
            "array_remove": (
                arr.array_remove(v), arr.filter(lambda x: x != v)),
            "slice": (
                arr.slice(col("s"), col("n")),
                arr.filter(lambda x, i: (i >= col("s0")) & (i < col("e")))),
            "array_repeat": (array_repeat(v, col("c")), None),
        }
        for case, (expr, base) in cases.items():
            _, out = timed(lambda: expr.eval(batch, schema))  # warm-up
            if base is not None:
                _, ref = timed(lambda: base.eval(batch, schema))
                if case == "array_position":
                    hit = out.data != 0
                    entry["position_hit_rows"] = int(hit.sum().item())
                    same = bool(torch.equal(hit, ref.data != 0))
                else:
                    entry[case + "_out_elements"] = out.child.size
                    same = _same_lists(out, ref)
                if not same:
                    raise SystemExit(f"{name} {case}: candidate and "
                                     "baseline disagree")
                del ref
            else:
                entry[case + "_out_elements"] = out.child.size
            del out
            tc, tb = [], []
            for _ in range(5):
                tc.append(timed(lambda: expr.eval(batch, schema))[0])
                if base is not None:
                    tb.append(timed(lambda: base.eval(batch, schema))[0])
            entry[case + "_ms"] = tc
            if base is not None:
                entry[case + "_base_ms"] = tb
        res[name] = entry
        print(name, json.dumps(entry), flush=True)
        del batch, a
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
