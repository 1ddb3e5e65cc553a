"""bench.py --dump-outputs: what the timed path computed in its last step, written as float64 .npy files so that two builds of
the project can be compared output for output.  CPU: the writer (file names, dtype, the size cap and its seeded sample).
GPU: the dump of a small fresh-columns run equals the rows of the same table fetched to the host (--dump-rows), and two runs
with the same arguments write the same bytes."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


def load_bench():
    spec = importlib.util.spec_from_file_location("tad_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fake_result(n, seed):
    rng = np.random.default_rng(seed)
    key = np.sort(rng.integers(0, 1000, n)).astype(np.uint64)
    return {"key_id": key, "flow_end_s": (1660202814 + 60 * rng.integers(0, 250, n)).astype(np.int64),
            "throughput": rng.integers(0, 2**40, n).astype(np.float64), "algo_calc": rng.normal(size=n), "stddev": rng.random(n)}


def test_dump_writes_every_column_as_float64(tmp_path):
    b = load_bench()
    res = fake_result(500, 1)
    b.dump_outputs(str(tmp_path), {"EWMA": res}, "", b.DUMP_LIMIT_BYTES)
    assert sorted(os.listdir(tmp_path)) == sorted(["EWMA_n_rows.npy"] + ["EWMA_%s.npy" % f for f in FIELDS])
    assert np.load(tmp_path / "EWMA_n_rows.npy").tolist() == [500.0]
    for f in FIELDS:
        got = np.load(tmp_path / ("EWMA_%s.npy" % f))
        assert got.dtype == np.float64
        assert np.array_equal(got, res[f].astype(np.float64)), f


def test_dump_above_the_limit_is_the_same_seeded_sample_of_every_column(tmp_path):
    b = load_bench()
    outputs = {"EWMA": fake_result(20000, 2), "ARIMA": fake_result(3000, 3)}
    limit = 200_000
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), outputs, "", limit)
    total = sum(os.path.getsize(tmp_path / "a" / fn) for fn in os.listdir(tmp_path / "a"))
    assert limit - 1000 < total <= limit
    for algo, cols in outputs.items():
        idx = np.load(tmp_path / "a" / ("%s_sample_index.npy" % algo)).astype(np.int64)
        assert idx.size < len(cols["key_id"]) and (np.diff(idx) > 0).all()
        assert np.load(tmp_path / "a" / ("%s_n_rows.npy" % algo)).tolist() == [float(len(cols["key_id"]))]
        for f in FIELDS:
            assert np.array_equal(np.load(tmp_path / "a" / ("%s_%s.npy" % (algo, f))), cols[f][idx].astype(np.float64)), (algo, f)
    for fn in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / fn).read_bytes() == (tmp_path / "b" / fn).read_bytes(), fn


def run_bench(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "2000000", "--keys", "2000", "--buckets", "100",
           "--no-cpu-baseline"] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_dump_is_the_last_timed_step_and_repeats(tmp_path):
    runs = []
    for d in ("d1", "d2"):
        line = run_bench(["--steps", "3", "--warmup", "1", "--tables", "4", "--dump-outputs", str(tmp_path / d)])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["tables"] == 4
        runs.append(line)
    assert runs[0]["result"] == runs[1]["result"]
    names = sorted(os.listdir(tmp_path / "d1"))
    assert names == sorted(os.listdir(tmp_path / "d2"))
    for fn in names:
        assert (tmp_path / "d1" / fn).read_bytes() == (tmp_path / "d2" / fn).read_bytes(), fn
    # the last timed step runs on table 0: its rows, fetched to the host by a separate run, are the dump
    run_bench(["--steps", "1", "--warmup", "1", "--dump-rows", str(tmp_path / "rows")])
    want = np.load(str(tmp_path / "rows") + ".rank0.npz")
    n = int(np.load(tmp_path / "d1" / "EWMA_n_rows.npy")[0])
    assert n == want["EWMA_key_id"].size == runs[0]["result"]["anomalies"] > 0
    for f in FIELDS:
        assert np.array_equal(np.load(tmp_path / "d1" / ("EWMA_%s.npy" % f)), want["EWMA_" + f].astype(np.float64), equal_nan=True), f
