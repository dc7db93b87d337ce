"""K JSON paths over one column: one fused get_json_object_multi call on this
tree, next to K get_json_object calls on another build of the project (the
parent commit, given as a directory that holds its `spark_rapids_amd` package
and built `hipdf` extension).

Shapes and generator: those of tools/bench_json_path.py (1,000,000 documents
of about 134 bytes, 50,000 of about 4 KB). Paths: the first K of PATHS, for
K = 2, 4, 8. Each figure is the backend call on a device column with a host
clock around a device synchronise; one warm-up each, then 5 repeats
alternating the fused call on this tree and the K calls on the other build.
This tree's own K single calls are recorded beside them for information only:
the baseline is the other build. Before a group is timed, the fused call's
columns are compared with this tree's single-path columns at the timed size
(lengths, bytes, validity); a difference ends the run.

Each build runs in a child process of its own. Without --other only this
tree is measured and the other build's figures are marked not measured.
Usage: python tools/bench_json_multi.py [out.json] [--other DIR]
(results recorded in profiles/r11_json_multi.md)."""
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_json_path import REPEATS, SHAPES, documents  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ["$.k", "$.s", "$.f", "$.b", "$.o.y", "$.o.x[1]", "$.a[2]",
         "$.missing"]
GROUP_SIZES = (2, 4, 8)


def worker(tree):
    sys.path.insert(0, tree)
    import torch
    from spark_rapids_amd import Column, DType
    from spark_rapids_amd.expr import json_path
    from spark_rapids_amd.ops import gpu_backend as g

    cols = {}

    def column(shape):
        if shape not in cols:
            nrows, pad = SHAPES[shape]
            cols[shape] = Column.from_pylist(documents(nrows, pad, 0),
                                             DType.string()).cuda()
        return cols[shape]

    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if cmd[0] == "quit":
            break
        c = column(cmd[1])
        if cmd[0] == "bytes":
            print(int(c.data.numel()), flush=True)
            continue
        paths = PATHS[:int(cmd[2])]
        if cmd[0] == "check":
            # the fused call's columns against the single-path call's, at
            # the size that is timed: lengths, bytes and validity
            fused = g.get_json_object_multi(
                c, [json_path.parse(p) for p in paths])
            for p, f in zip(paths, fused):
                one = g.get_json_object(c, p)
                fo, oo = f.offsets.long(), one.offsets.long()
                assert torch.equal(fo - fo[0], oo - oo[0]), p
                assert torch.equal(f.data[int(fo[0]):int(fo[-1])],
                                   one.data[int(oo[0]):int(oo[-1])]), p
                nb = c.size // 8
                assert torch.equal(f.validity[:nb], one.validity[:nb]), p
            print(1, flush=True)
            continue
        if cmd[3] == "multi":
            steps = [json_path.parse(p) for p in paths]
            fn = lambda: g.get_json_object_multi(c, steps)
        else:
            fn = lambda: [g.get_json_object(c, p) for p in paths]
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
        self.p.stdin.write(" ".join(str(w) for w in words) + "\n")
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
                     "column_bytes": int(new.ask("bytes", shape))}
            for k in GROUP_SIZES:
                new.ask("check", shape, k)
                new.ask("run", shape, k, "multi")  # warm-up
                new.ask("run", shape, k, "single")
                if other:
                    other.ask("run", shape, k, "single")
                fused, own, base = [], [], []
                for _ in range(REPEATS):
                    fused.append(new.ask("run", shape, k, "multi"))
                    if other:
                        base.append(other.ask("run", shape, k, "single"))
                    own.append(new.ask("run", shape, k, "single"))
                entry[f"k{k}_fused_ms"] = fused
                entry[f"k{k}_other_single_calls_ms"] = \
                    base if other else "not measured"
                entry[f"k{k}_this_tree_single_calls_ms"] = own
                print(shape, k, fused, base, own, flush=True)
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
