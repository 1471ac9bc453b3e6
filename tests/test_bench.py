"""bench.py command line: --steps is honoured, the result line carries
ms_per_step, and --dump-outputs writes the last step's merged columns
reproducibly (tiny CPU scenario, in-process)."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(monkeypatch, capsys, tmp_path, tag, extra=()):
    sys.path.insert(0, ROOT)
    import bench

    out = tmp_path / f"out_{tag}"
    monkeypatch.setenv("LAKESOUL_META_DB", "")  # restored after the test
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
        "--device", "cpu", "--rows-base", "20000", "--rows-upsert", "2000",
        "--upserts", "2", "--buckets-per-gpu", "4",
        "--workdir", str(tmp_path / f"wd_{tag}"),
        "--dump-outputs", str(out), *extra])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines()
             if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_dump_outputs_reproducible(monkeypatch, capsys, tmp_path):
    res_a, out_a = _run_bench(monkeypatch, capsys, tmp_path, "a")
    res_b, out_b = _run_bench(monkeypatch, capsys, tmp_path, "b", ["--full"])

    assert res_a["steps"] == 2 and res_a["ms_per_step"] > 0
    for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert key in res_a
    rows = res_a["config"]["merged_rows_per_step_per_gpu"]
    assert rows == 20000  # upserts hit existing PKs: merge dedups them

    names = sorted(os.listdir(out_a))
    assert names == sorted(os.listdir(out_b))
    assert {"id.npy", "v.npy", "k.npy", "f.npy", "t.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(out_a / n), np.load(out_b / n)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 10**6
    ids = np.load(out_a / "id.npy")
    assert len(ids) == rows and len(np.unique(ids)) == rows
