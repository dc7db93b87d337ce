"""transform / filter / exists over LIST<int64> next to the work they are made
of: (a) transform(a, x -> x * 2 + 1) and (b) transform(a, x -> x + k) against
the same two elementwise ops on the flat child, (c) filter(a, x -> x % 3 = 0)
against array_distinct(a), (d) exists(a, x -> x > c), c the median row
maximum so that about half the rows hold a hit, against the compare alone on
the flat child. Expressions are evaluated on a device batch directly; one
warm-up, then 5 repeats alternating candidate and baseline inside one
process, host clock around a device synchronise.
Usage: python tools/bench_list_lambda.py [out.json]
(results recorded in profiles/r09_array_lambda.md)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_amd import (Column, ColumnBatch, DType, Field,  # noqa: E402
                              Schema, col)
from spark_rapids_amd.ops import gpu_backend as g  # noqa: E402

I64 = DType.int64()
L_I64 = DType.list_(I64)


def make(nrows, lo, hi, seed):
    """(device batch [a, k], schema, median row maximum)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, nrows).astype(np.int64)
    offs = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[-1])
    vals = rng.integers(0, 1 << 40, total, dtype=np.int64)
    rowmax = np.full(nrows, -1, dtype=np.int64)
    full = lens > 0
    rowmax[full] = np.maximum.reduceat(vals, offs[:-1][full])
    child = Column(I64, total, torch.from_numpy(vals).cuda(), None,
                   null_count=0)
    a = Column(L_I64, nrows, torch.zeros(0, dtype=torch.uint8, device="cuda"),
               None, torch.from_numpy(offs.astype(np.int32)).cuda(), 0, child)
    k = Column(I64, nrows,
               torch.from_numpy(rng.integers(0, 100, nrows)).cuda(), None,
               null_count=0)
    schema = Schema([Field("a", L_I64), Field("k", I64)])
    return ColumnBatch([a, k], nrows), schema, int(np.median(rowmax))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    res = {}
    for name, nrows, lo, hi in (("short_4M_len0-16", 4_000_000, 0, 16),
                                ("block_64K_len900-1100", 65_536, 900, 1100)):
        batch, schema, c = make(nrows, lo, hi, 1)
        a = batch.columns[0]
        child = a.child
        mean_len = -(-child.size // nrows)
        entry = {"rows": nrows, "elements": child.size, "exists_bound": c,
                 "bool_reduce_width": g._list_group_width(mean_len)}

        def flat_mul_add():
            return g.binary_op_scalar(
                "add", g.binary_op_scalar("mul", child, 2, I64), 1, I64)

        cases = {
            "transform_mul_add": (
                col("a").transform(lambda x: x * 2 + 1), flat_mul_add),
            "transform_outer": (
                col("a").transform(lambda x: x + col("k")), flat_mul_add),
            "filter_mod3": (
                col("a").filter(lambda x: x % 3 == 0),
                lambda: g.array_distinct(a)),
            "exists_gt": (
                col("a").exists(lambda x: x > c),
                lambda: g.binary_op_scalar("gt", child, c, DType.bool_())),
        }
        for case, (expr, base) in cases.items():
            _, out = timed(lambda: expr.eval(batch, schema))  # warm-up
            timed(base)
            if case == "filter_mod3":
                entry["filter_out_elements"] = out.child.size
            if case == "exists_gt":
                entry["exists_true_rows"] = int(out.data.sum().item())
            del out
            tc, tb = [], []
            for _ in range(5):
                tc.append(timed(lambda: expr.eval(batch, schema))[0])
                tb.append(timed(base)[0])
            entry[case + "_ms"] = tc
            entry[case + "_base_ms"] = tb
        res[name] = entry
        print(name, json.dumps(entry), flush=True)
        del batch, a, child
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
