"""array_intersect / array_union / arrays_overlap next to array_distinct of
the left operand. Two LIST<int64> operands with about half their values
shared; one warm-up, then 5 repeats alternating the set operation with
array_distinct inside one process, host clock around a device synchronise.
Usage: python tools/bench_list_setops.py [out.json]
(results recorded in profiles/r08_array_setops.md)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_amd import Column, DType  # noqa: E402
from spark_rapids_amd.ops import gpu_backend as g  # noqa: E402


def make(nrows, lo, hi, seed):
    """Two operands over the same rows, both drawn from [0, D) with
    D = 1.44 x the mean length: an element then has an equal one in a row
    of mean length on the other side with probability about one half."""
    rng = np.random.default_rng(seed)
    domain = max(2, round(1.44 * (lo + hi) / 2))
    cols = []
    for _ in range(2):
        lens = rng.integers(lo, hi + 1, nrows).astype(np.int64)
        offs = np.zeros(nrows + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        total = int(offs[-1])
        vals = rng.integers(0, domain, total, dtype=np.int64)
        child = Column(DType.int64(), total, torch.from_numpy(vals).cuda(),
                       None, null_count=0)
        o32 = torch.from_numpy(offs.astype(np.int32)).cuda()
        cols.append(Column(DType.list_(DType.int64()), nrows,
                           torch.zeros(0, dtype=torch.uint8, device="cuda"),
                           None, o32, 0, child))
    return cols


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
        a, b = make(nrows, lo, hi, 1)
        entry = {"rows": nrows, "a_elements": a.child.size,
                 "b_elements": b.child.size,
                 "distinct_a_elements": g.array_distinct(a).child.size}
        for op in ("array_intersect", "array_union", "arrays_overlap"):
            fn = getattr(g, op)
            _, out = timed(lambda: fn(a, b))       # warm-up
            timed(lambda: g.array_distinct(a))
            if op == "arrays_overlap":
                entry["overlap_true_rows"] = int(out.data.sum().item())
            else:
                entry[op + "_out_elements"] = out.child.size
            del out
            ts, td = [], []
            for _ in range(5):
                ts.append(timed(lambda: fn(a, b))[0])
                td.append(timed(lambda: g.array_distinct(a))[0])
            entry[op + "_ms"] = ts
            entry[op + "_distinct_ms"] = td
        res[name] = entry
        print(name, json.dumps(entry), flush=True)
        del a, b
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
