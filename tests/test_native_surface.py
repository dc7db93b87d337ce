"""Every attribute the Python sources read on the native extension must exist
on the built module: a binding dropped from hipdf_module.cpp fails here,
without a GPU."""
import ast
import os

import hipdf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "spark_rapids_amd")


def _is_extension(node: ast.expr) -> bool:
    """`ext`, `hipdf`, or anything ending in `.ext` (self.ext, gb.ext)."""
    if isinstance(node, ast.Name):
        return node.id in ("ext", "hipdf")
    return isinstance(node, ast.Attribute) and node.attr == "ext"


def _extension_reads():
    reads = {}  # name -> first "file:line" that reads it
    for root, _, files in os.walk(PKG):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(root, f)
            with open(path, encoding="utf-8") as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if (isinstance(node, ast.Attribute)
                        and isinstance(node.ctx, ast.Load)
                        and _is_extension(node.value)):
                    where = f"{os.path.relpath(path, REPO)}:{node.lineno}"
                    reads.setdefault(node.attr, where)
    return reads


def test_every_extension_attribute_read_exists():
    reads = _extension_reads()
    # the walk found the call sites at all: the flagship kernels are there
    for known in ("binary_arith", "sort_order", "gb_agg_multi", "pool_used",
                  "rle_hybrid_batch", "memcpy_h2d"):
        assert known in reads, f"walk missed {known}"
    missing = {n: w for n, w in reads.items() if not hasattr(hipdf, n)}
    assert not missing, f"read in python but not bound: {missing}"
