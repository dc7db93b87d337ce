"""bench.py command line: a plain run times only the steps; --full adds the
CPU-backend baseline; --dump-outputs writes the last step's results."""
import glob
import json
import os
import subprocess
import sys
from decimal import Decimal

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_column_array_encoding():
    sys.path.insert(0, REPO)
    import bench

    a, k = bench._column_arrays(
        [1, None, Decimal("2.50"), 3.25, True, float("nan"), float("inf"),
         float("-inf")])
    assert a.dtype == np.float64 and k.dtype == np.float64
    assert np.array_equal(a, [1.0, 0.0, 2.5, 3.25, 1.0, 0.0, 0.0, 0.0])
    assert np.array_equal(k, [0, 1, 0, 0, 0, 2, 3, 4])
    s, k = bench._column_arrays(["ab", "ab", "ac", None])
    assert s[0] == s[1] != s[2] and s[3] == 0.0
    assert np.array_equal(k, [0, 0, 0, 1])
    a, k = bench._column_arrays([])
    assert a.shape == (0,) and k.shape == (0,)


def _run_bench(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
           "--warmup", "0", "--rows-per-gpu", "100000", "--partitions", "2",
           "--data-dir", str(tmp_path / "data"), *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path):
    out = tmp_path / "dump"
    res = _run_bench(tmp_path, "--steps", "2", "--dump-outputs", str(out))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in res
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    # the CPU baseline is not measured without --full
    assert res["vs_baseline"] is None
    assert res["config"]["speedup_vs_cpu_backend"] is None
    files = sorted(glob.glob(str(out / "*.npy")))
    assert {os.path.basename(f).split(".")[0] for f in files} == set(
        res["config"]["queries"])
    arrays = [np.load(f) for f in files]
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in arrays)
    assert sum(a.nbytes for a in arrays) <= 64 << 20
    # NULLs (the rollup queries produce them) are marked in .kind.npy, so
    # every written value is finite
    assert all(np.isfinite(a).all() for a in arrays)
    assert any(a.size and a.any() for a in arrays)
    for f in files:
        if not f.endswith(".kind.npy"):
            assert os.path.exists(f[:-len(".npy")] + ".kind.npy"), f
    q67_cat = [f for f in files
               if os.path.basename(f).startswith("q67.00_")
               and f.endswith(".kind.npy")]
    assert len(q67_cat) == 1 and (np.load(q67_cat[0]) == 1).any()

    # same arguments -> same inputs -> same results, output for output.
    # Row order is compared only where the query's sort keys determine it
    # (the others can reorder rows whose float sort key ties); float sums
    # reassociate under atomics, hence the 1e-9 relative tolerance used
    # for concurrent sums elsewhere in the suite.
    ordered = {"q3", "q42", "q52", "q55", "q7", "q96"}
    out2 = tmp_path / "dump2"
    _run_bench(tmp_path, "--steps", "1", "--dump-outputs", str(out2))
    for f, a in zip(files, arrays):
        b = np.load(out2 / os.path.basename(f))
        assert a.shape == b.shape
        if os.path.basename(f).split(".")[0] in ordered:
            assert np.allclose(a, b, rtol=1e-9, atol=0.0, equal_nan=True), f


@pytest.mark.gpu
def test_full_run_measures_cpu_baseline(tmp_path):
    res = _run_bench(tmp_path, "--steps", "1", "--full",
                     "--cpu-baseline-procs", "2")
    assert res["config"]["speedup_vs_cpu_backend"] > 0
    assert res["vs_baseline"] == pytest.approx(
        res["config"]["speedup_vs_cpu_backend"] / 3.0)
