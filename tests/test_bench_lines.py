"""bench.py: a plain run is the headline alone; --full adds what the headline does not need, after it, in the same process.
CPU: the option exists.  GPU: the default C2 line without and with --full (the extra configs and CPU baselines trimmed)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("same_columns", "other_configs", "concurrency", "row_orders", "cpu_baseline")


def test_full_is_an_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout


def run_line(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines and lines[-1].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[-1])


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone():
    d = run_line([])
    for f in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert f in d, f
    assert d["metric"] == "flow-records/sec" and d["unit"] == "flow-records/s" and d["higher_is_better"] is True
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["tables"] == 4 and d["config"]["baseline_config"] == "c2"
    assert abs(d["value"] - 100_000_000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    assert d["roofline"]["frac"] > 0 and d["cold"]["ms_first_step"] > 0 and d["result"]["anomalies"] > 0
    for f in EXTRAS:
        assert f not in d, f


@pytest.mark.gpu
def test_full_line_adds_the_extras_after_the_same_headline():
    plain = run_line([])
    full = run_line(["--full", "--no-other-configs", "--no-cpu-baseline"])
    assert full["result"] == plain["result"] and full["config"] == plain["config"]
    assert full["same_columns"]["steps"] == 1 and full["same_columns"]["ms_per_step"] > 0
    for f in EXTRAS[1:]:
        assert f not in full, f
