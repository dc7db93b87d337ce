"""sort_array tiers vs the composed path (sort_order over (row id, value) +
gather). Alternates candidates, 5 repeats after a warm-up, host clock around
a device synchronise. Usage: python tools/bench_list_sort.py [out.json]
(results recorded in profiles/r05_list_sort.md)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_amd import Column, ColumnBatch, DType  # noqa: E402
from spark_rapids_amd.ops import gpu_backend as g  # noqa: E402


def make(nrows, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, nrows).astype(np.int64)
    offs = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[-1])
    vals = rng.integers(-2 ** 62, 2 ** 62, total, dtype=np.int64)
    child = Column(DType.int64(), total, torch.from_numpy(vals).cuda(), None,
                   null_count=0)
    o32 = torch.from_numpy(offs.astype(np.int32)).cuda()
    col = Column(DType.list_(DType.int64()), nrows,
                 torch.zeros(0, dtype=torch.uint8, device="cuda"), None, o32,
                 0, child)
    seg = torch.repeat_interleave(
        torch.arange(nrows, device="cuda", dtype=torch.int32),
        torch.from_numpy(lens).cuda())
    return col, seg, total


def composed(col, seg):
    m = col.child.size
    segc = Column(DType.int32(), m, seg, None, null_count=0)
    order = g.sort_order(ColumnBatch([segc, col.child], m), [0, 1],
                         [False, False], [False, False])
    return g._gather_col(col.child, order.data, m, maybe_negative=False)


def new(col):
    return g.sort_array(col, True, True).child


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
        col, seg, total = make(nrows, lo, hi, 1)
        _, a = timed(lambda: new(col))          # warm-up + equality
        _, b = timed(lambda: composed(col, seg))
        same = bool((a.data == b.data).all())
        tn, tc = [], []
        for _ in range(5):
            tn.append(timed(lambda: new(col))[0])
            tc.append(timed(lambda: composed(col, seg))[0])
        res[name] = {"rows": nrows, "elements": total, "same_result": same,
                     "new_ms": tn, "composed_ms": tc}
        print(name, json.dumps(res[name]), flush=True)
        del col, seg, a, b
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
