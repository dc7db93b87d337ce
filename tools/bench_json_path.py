"""get_json_object on the device, next to the same call on another build of
the project (the parent commit, given as a directory that holds its
`spark_rapids_amd` package and built `hipdf` extension).

Shapes: 1,000,000 generated documents of about 120 bytes (the fields of the
generator in tests/test_strings.py plus one nested object and one array) and
50,000 documents of about 4 KB (the same with a long array in the middle).

Cases, each the backend call on a device column, host clock around a device
synchronise, one warm-up then 5 repeats alternating this tree and the other:
  a  `$.k`        top-level scalar: both builds answer on the device
  b  `$.o.x[1]`   nested path: the other build copies the column to the host
                  and runs a Python loop
  c  `$.o.x[1]`   as b on a column where 1% of the rows spell that number
                  `1e2`, which the device hands to the host (this tree only)
  size           the size-pass launch alone (this tree only)

Each build runs in a child process of its own. Without --other only this
tree is measured and the other build's figures are marked not measured.
Usage: python tools/bench_json_path.py [out.json] [--other DIR]
(results recorded in profiles/r10_json_path.md)."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"short_1M_120B": (1_000_000, 0), "long_50K_4KB": (50_000, 480)}
CASES = {"a": ("plain", "$.k"), "b": ("plain", "$.o.x[1]"),
         "c": ("flag1pct", "$.o.x[1]"), "size": ("plain", "$.o.x[1]")}
REPEATS = 5


def documents(nrows, pad, flag_every):
    """Deterministic: row i is a function of i. flag_every > 0 spells
    x[1] of every flag_every-th row as 1e2."""
    rows = []
    t = ", ".join(str(100000 + j) for j in range(pad))
    for i in range(nrows):
        x1 = "1e2" if flag_every and i % flag_every == 0 else str(i + 1)
        rows.append(
            '{"k": %d, "s": "v%d", "f": %s, "b": %s, "t": [%s], '
            '"o": {"x": [%d, %s, %d], "y": "n%d"}, "a": [1, 2, 3]}'
            % (i, i, repr(i / 4), "true" if i % 2 else "false", t,
               i, x1, i * 2, i))
    return rows


def worker(tree):
    sys.path.insert(0, tree)
    import torch
    from spark_rapids_amd import Column, DType
    from spark_rapids_amd.ops import cpu_backend, gpu_backend as g

    cols = {}
    host_only = set()

    def column(shape, kind):
        if (shape, kind) not in cols:
            nrows, pad = SHAPES[shape]
            rows = documents(nrows, pad, 100 if kind == "flag1pct" else 0)
            cols[shape, kind] = Column.from_pylist(rows,
                                                   DType.string()).cuda()
        return cols[shape, kind]

    def size_pass(c, path):
        from spark_rapids_amd.expr import json_path

        flat, names = json_path.encode(json_path.parse(path))
        st = torch.tensor(flat, dtype=torch.int32).cuda()
        nm = torch.frombuffer(bytearray(names), dtype=torch.uint8).cuda()
        n = c.size
        lens = torch.empty(n, dtype=torch.int64, device="cuda")
        ss = torch.empty(n, dtype=torch.int32, device="cuda")
        sl = torch.empty(n, dtype=torch.int32, device="cuda")
        state = torch.empty(n, dtype=torch.uint8, device="cuda")

        def run():
            g.ext.json_path(c.offsets.data_ptr(), c.data.data_ptr(), 0,
                            st.data_ptr(), nm.data_ptr(), len(flat) // 3, 0,
                            lens.data_ptr(), ss.data_ptr(), sl.data_ptr(),
                            state.data_ptr(), 0, 0, n, g._stream())
            return state
        return run

    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if cmd[0] == "quit":
            break
        shape, case = cmd[1], cmd[2]
        kind, path = CASES[case]
        c = column(shape, kind)
        if cmd[0] == "bytes":
            print(int(c.data.numel()), flush=True)
            continue
        if case == "size":
            fn = size_pass(c, path)
        elif (case, tree) in host_only:
            # what the plan does with an expression tagged to the CPU: copy
            # the column to the host and call the host backend
            fn = lambda: cpu_backend.get_json_object(c.cpu(), path)
        else:
            fn = lambda: g.get_json_object(c, path)
            try:
                g.get_json_object(Column.from_pylist(["{}"],
                                                     DType.string()).cuda(),
                                  path)
            except NotImplementedError:  # a build without the path kernel
                host_only.add((case, tree))
                fn = lambda: cpu_backend.get_json_object(c.cpu(), path)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        del out
        print(f"{ms:.4f}", flush=True)


class Child:
    def __init__(self, tree):
        self.p = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--worker", tree],
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self.p.stdout.readline().strip() == "ready"

    def ask(self, *words):
        self.p.stdin.write(" ".join(words) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("worker ended")
        return float(line)

    def close(self):
        if self.p.poll() is None:
            self.p.stdin.write("quit\n")
            self.p.stdin.close()
        self.p.wait()


def main():
    args = sys.argv[1:]
    other_tree = None
    if "--other" in args:
        i = args.index("--other")
        other_tree = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    new = Child(REPO)
    other = Child(other_tree) if other_tree else None
    res = {}
    try:
        for shape, (nrows, _) in SHAPES.items():
            entry = {"rows": nrows,
                     "column_bytes": int(new.ask("bytes", shape, "a")),
                     "flag1pct_column_bytes":
                         int(new.ask("bytes", shape, "c"))}
            for case in CASES:
                both = other is not None and case in ("a", "b")
                new.ask("run", shape, case)  # warm-up
                if both:
                    other.ask("run", shape, case)
                tn, to = [], []
                for _ in range(REPEATS):
                    tn.append(new.ask("run", shape, case))
                    if both:
                        to.append(other.ask("run", shape, case))
                entry[case + "_ms"] = tn
                entry[case + "_other_ms"] = to if both else "not measured"
                print(shape, case, tn, to, flush=True)
            res[shape] = entry
    finally:
        new.close()
        if other:
            other.close()
    print(json.dumps(res), flush=True)
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        main()
