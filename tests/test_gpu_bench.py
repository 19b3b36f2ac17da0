"""bench.py's two kinds of run, on a small workload: a plain run does only what its headline needs (set-up, warm-up, timed steps,
--dump-outputs, the line), `--full` adds everything else.  Both must write the same flows -- the DeepFlow leg's included, which a plain
run does not time but still dumps -- so that a plain run can stand in for a full one in an output-for-output comparison of two builds.

Each run is a child process: bench.py imports torch before the engine, and in the pytest process the engine's fixture may already
have initialised HIP."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "10", "--sub-batch", "4", "--size", "128", "--steps", "2",
                        "--warmup", "1"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_flows(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for d in (plain, full):
        assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["steps"] == 2 and d["warmup"] == 1
        assert d["metric"] == "frame-pairs/sec @512x512 DualTVL1" and d["unit"] == "frame-pairs/s" and d["higher_is_better"] is True
    # the plain line: the timed steps and nothing measured beside them
    assert plain["full"] is False
    for k in ("roofline", "steps_joined", "jobs_in_flight", "latency_ms_single_pair", "pcie_inclusive_pairs_per_s", "saliency", "stage_ms_per_step"):
        assert k not in plain, k
    assert "value" not in plain["deepflow"] and plain["deepflow"]["dumped_outputs"]["file"] == "deepflow_flows.npy"
    # the full line: the rest, the DeepFlow leg timed
    assert full["full"] is True
    for k in ("roofline", "steps_joined", "jobs_in_flight", "latency_ms_single_pair", "pcie_inclusive_pairs_per_s", "saliency", "stage_ms_per_step"):
        assert k in full, k
    assert full["deepflow"]["value"] > 0 and full["deepflow"]["steps"] == 2
    for name, rp, rf in (("tvl1_flows.npy", plain["dumped_outputs"], full["dumped_outputs"]),
                         ("deepflow_flows.npy", plain["deepflow"]["dumped_outputs"], full["deepflow"]["dumped_outputs"])):
        assert rp == rf and rp["file"] == name and rp["shape"] == [10, 128, 128, 2]
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b), f"{name}: a plain run dumped other flows than a full run"
