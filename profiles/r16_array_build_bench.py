"""Times array(), concat over arrays, flatten, sequence and array_join on the
GPU at 10M rows of short rows (k = 4 for array(), lengths 0-8 elsewhere),
each as the backend op on device columns: one warm-up, then 7 runs, host
clock around a device synchronise. Next to each time stands the bytes the
op has to move at the least (operands read once, result written once,
computed from the shapes below) and the rate that makes.

The parent commit has no device path for any of them: there such a column is
built on the host with Column.from_pylist and uploaded. That is timed here
for the same kind of rows at 1M rows (python lists ready before the clock
starts) and scaled by 10, labelled as scaled.

Usage: python profiles/r16_array_build_bench.py [out.json]
(results recorded in profiles/r16_array_build.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_amd import Column, DType  # noqa: E402
from spark_rapids_amd.ops import gpu_backend as g  # noqa: E402

I32, I64, STR = DType.int32(), DType.int64(), DType.string()
L = DType.list_
N_DEV, N_HOST, RUNS = 10_000_000, 1_000_000, 7
NO_DATA = dict(dtype=torch.uint8, device="cuda")


def fixed(t, dt):
    return Column(dt, t.numel(), t, None, null_count=0)


def offsets(rng, n, hi=8):
    lens = rng.integers(0, hi + 1, n)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs.astype(np.int32)


def int_list(rng, n):
    offs = offsets(rng, n)
    vals = torch.randint(0, 1 << 40, (int(offs[-1]),), device="cuda")
    return Column(L(I64), n, torch.zeros(0, **NO_DATA), None,
                  torch.from_numpy(offs).cuda(), 0, fixed(vals, I64))


def str_list(rng, n):
    """LIST<STRING>, 0-8 strings of 0-8 letters per row."""
    offs = offsets(rng, n)
    m = int(offs[-1])
    eoffs = offsets(rng, m)
    data = torch.randint(97, 123, (int(eoffs[-1]),), dtype=torch.uint8,
                         device="cuda")
    child = Column(STR, m, data, None, torch.from_numpy(eoffs).cuda(), 0)
    return Column(L(STR), n, torch.zeros(0, **NO_DATA), None,
                  torch.from_numpy(offs).cuda(), 0, child)


def nested_list(rng, n):
    offs = offsets(rng, n)
    inner = int_list(rng, int(offs[-1]))
    return Column(L(L(I64)), n, torch.zeros(0, **NO_DATA), None,
                  torch.from_numpy(offs).cuda(), 0, inner)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def cases(rng, n):
    """name -> (callable, least bytes moved)."""
    out = {}
    cols = [fixed(torch.randint(0, 1 << 40, (n,), device="cuda"), I64)
            for _ in range(4)]
    out["array_k4_int64"] = (lambda: g.create_array(cols),
                             2 * 4 * n * 8 + 4 * (n + 1))
    a, b = int_list(rng, n), int_list(rng, n)
    elems = a.child.size + b.child.size
    out["concat_2_int64"] = (lambda: g.array_concat([a, b]),
                             2 * 4 * (n + 1) + 2 * 8 * elems + 4 * (n + 1))
    nest = nested_list(rng, n)
    # the innermost child is reused: only offsets move
    out["flatten_int64"] = (lambda: g.array_flatten(nest),
                            4 * (n + 1) + 4 * (n + 1) + 4 * (n + 1))
    start = fixed(torch.randint(0, 1000, (n,), device="cuda"), I64)
    stop = fixed(start.data + torch.randint(0, 8, (n,), device="cuda"), I64)
    seq_elems = int((stop.data - start.data).sum().item()) + n
    out["sequence_int64"] = (lambda: g.sequence(start, stop),
                             2 * 8 * n + 8 * seq_elems + 4 * (n + 1))
    s = str_list(rng, n)
    nbytes, m = s.child.data.numel(), s.child.size
    joined = nbytes + max(m - n, 0)  # about one delimiter between elements
    out["array_join"] = (lambda: g.array_join(s, ","),
                         4 * (n + 1) + 4 * (m + 1) + nbytes + joined +
                         4 * (n + 1))
    return out


def host_cases(rng, n):
    """The same kinds of rows as python lists, and their types."""
    def lists(hi=8):
        lens = rng.integers(0, hi + 1, n)
        return [rng.integers(0, 1 << 40, int(k)).tolist() for k in lens]

    words = ["", "a", "bc", "def", "ghij", "klmno", "pqrstu", "vwxyzab",
             "cdefghij"]
    strs = [[words[int(x)] for x in rng.integers(0, 9, int(k))]
            for k in rng.integers(0, 9, n)]
    a, b = lists(), lists()
    return {
        "array_k4_int64": ([list(r) for r in
                            rng.integers(0, 1 << 40, (n, 4)).tolist()],
                           L(I64)),
        "concat_2_int64": ([x + y for x, y in zip(a, b)], L(I64)),
        "flatten_int64": ([x + y for x, y in zip(a, b)], L(I64)),
        "sequence_int64": ([list(range(int(x), int(x) + int(k) + 1))
                            for x, k in zip(rng.integers(0, 1000, n),
                                            rng.integers(0, 8, n))], L(I64)),
        "array_join": ([",".join(r) for r in strs], STR),
    }


def main():
    rng = np.random.default_rng(16)
    res = {"rows": N_DEV, "host_rows": N_HOST, "runs": RUNS,
           "device": torch.cuda.get_device_name(0)}
    for name, (fn, nbytes) in cases(rng, N_DEV).items():
        timed(fn)  # warm-up
        ms = [timed(fn)[0] for _ in range(RUNS)]
        med = statistics.median(ms)
        res[name] = {"gpu_ms": ms, "gpu_median_ms": med,
                     "least_bytes": nbytes,
                     "gbytes_per_s": nbytes / med / 1e6}
        print(name, json.dumps(res[name]), flush=True)
        torch.cuda.empty_cache()
    for name, (rows, dt) in host_cases(rng, N_HOST).items():
        def build():
            return Column.from_pylist(rows, dt).cuda()
        timed(build)
        ms = [timed(build)[0] for _ in range(5)]
        med = statistics.median(ms)
        res[name].update(host_1m_ms=ms, host_1m_median_ms=med,
                         host_scaled_to_10m_ms=med * N_DEV / N_HOST)
        print(name, "host", json.dumps(ms), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
