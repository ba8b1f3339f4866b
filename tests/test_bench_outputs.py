"""bench.py --dump-outputs / --full: the writer of the last timed step's outputs (float32 / float64 files, one seeded
sample of the batch rows for every array above the size limit, the same from run to run), checked on the CPU; and on the
GPU that a plain run keeps the --full-only figures out of its line while --dump-outputs writes the same arrays twice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_keeps_small_outputs_whole(tmp_path):
    b = _bench()
    u = np.arange(7 * 3, dtype=np.float64).reshape(7, 3)
    u32 = u.astype(np.float32)
    st = np.arange(7, dtype=np.int32)
    b.dump_outputs(str(tmp_path / "d"), 0, {"u": u, "u32": u32, "status": st})
    assert sorted(os.listdir(tmp_path / "d")) == ["status.npy", "u.npy", "u32.npy"]
    got = {k: np.load(tmp_path / "d" / f"{k}.npy") for k in ("u", "u32", "status")}
    assert got["u"].dtype == np.float64 and got["u32"].dtype == np.float32 and got["status"].dtype == np.float64
    assert np.array_equal(got["u"], u) and np.array_equal(got["u32"], u32) and np.array_equal(got["status"], st)


def test_dump_outputs_samples_the_same_rows_of_every_array_under_the_limit(tmp_path):
    b = _bench()
    B = 50
    u = np.random.default_rng(1).standard_normal((B, 4, 3))
    st = np.arange(B, dtype=np.int32)
    limit = 1000  # bytes: 96 + 8 + 8 per row -> 8 rows
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), 0, {"u": u, "status": st}, limit=limit)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("u", "status", "rows")}
    rows = a["rows"].astype(int)
    assert len(rows) == 8 and len(set(rows)) == 8 and np.all(np.diff(rows) > 0) and rows.max() < B
    assert np.array_equal(a["u"], u[rows]) and np.array_equal(a["status"], st[rows])
    assert sum(v.nbytes for v in a.values()) <= limit
    for k, v in a.items():  # the sample is fixed: a second run writes the same files
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), v)


def test_dump_outputs_other_ranks_write_their_own_files(tmp_path):
    b = _bench()
    b.dump_outputs(str(tmp_path), 1, {"u": np.zeros((2, 3))})
    assert os.listdir(tmp_path) == ["u.rank1.npy"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "256",
                            "--min-warmup-s", "0", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 3 and d["full"] is False and d["ms_per_step"] > 0
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert d["value_short_warmup"] is None and d["value_end_to_end"] is None
    assert "cpu_baseline" not in d and "max_rel_du_vs_cpu_fp64" not in d
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("u", "status", "iters")}
    assert a["u"].shape == (256, 10, 4, 3) and a["u"].dtype == np.float64
    assert np.all(a["status"] == 0) and np.all(a["iters"] > 0) and np.all(np.isfinite(a["u"]))
    for k, v in a.items():
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), v), k
