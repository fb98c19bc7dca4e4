"""bench.py keeps the driver's contract: one JSON line with the required keys (a
plain run: the primary line alone, and the table it dumps); with --full a roofline
object and a CPU baseline too, on a small workload (a child process each)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_and_dump(oracle, tmp_path):
    """A plain run prints the primary line alone (no leg of --full), takes --steps timed
    steps, and --dump-outputs writes the table of the last timed build: float64 / float32
    arrays, every cell equal to the oracle's table of the same seeded graph."""
    import numpy as np

    from shadow_amd import synth

    n = 300
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--nodes", str(n), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["full"] is False
    assert abs(d["ms_per_step"] - d["value"] * 1e3) < 1e-3
    for k in ("delivery", "codel", "inbound", "outbound", "c2", "gml_ingest", "apsp_detail"):
        assert k not in d, k
    assert d["roofline"] is None and d["cpu_baseline"] is None
    lat = np.load(tmp_path / "out" / "latency_ns.npy")
    loss = np.load(tmp_path / "out" / "packet_loss.npy")
    assert sorted(os.listdir(tmp_path / "out")) == ["latency_ns.npy", "packet_loss.npy"]
    assert lat.dtype == np.float64 and loss.dtype == np.float32 and lat.shape == loss.shape == (n * n,)
    g = synth.ring_chords_graph(n, 8.0, seed=1)
    rc, olat, oloss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], False,
                                               np.arange(n, dtype=np.uint32), threads=4)
    assert rc == 0
    assert np.array_equal(lat, olat.ravel().astype(np.float64))
    assert np.array_equal(loss.view(np.uint32), oloss.ravel().view(np.uint32))


def test_bench_json_contract():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--nodes", "1000",
           "--hosts", "5000", "--packets", "50000", "--no-gml", "--no-c2"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["config"]["workload"] and "model" not in d["config"]
    dl = d["delivery"]
    assert dl["value"] > 0 and dl["roofline"]["bound"] == "hbm" and dl["cpu_baseline"]["cores"] >= 1
    assert d["inbound"]["parity_vs_cpu"] is True
