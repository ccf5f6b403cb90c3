"""bench.py's plain run and `--dump-outputs DIR`: a plain run prints the headline line only (the CPU baseline, the clock readings and the
`extras` child runs come with `--full`), `--steps` is the number of timed steps, and two runs with the same arguments write the same
arrays -- what the timed steps computed -- as float64 .npy files of at most 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _run(*args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, *args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_sample_is_fixed_and_fits():
    a, b = bench.dump_sample(10**6, 124 * 8), bench.dump_sample(10**6, 124 * 8)
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10**6
    assert a.size * (124 * 8 + 8) <= bench.DUMP_MAX_BYTES - (1 << 20)
    np.testing.assert_array_equal(bench.dump_sample(1000, 124 * 8), np.arange(1000))


def test_write_outputs_keeps_to_its_budget(tmp_path):
    bench.write_outputs(str(tmp_path / "ok"), {"x": np.arange(5, dtype=np.int32), "y": np.ones(3, dtype=np.float32)})
    got = _load(str(tmp_path / "ok"))
    assert got["x"].dtype == np.float64 and got["y"].dtype == np.float32
    np.testing.assert_array_equal(got["x"], np.arange(5))
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    args = ("--gpus", "1", "--steps", "6", "--warmup", "2", "--size", "256", "250")
    runs = []
    for tag in ("a", "b"):
        rec = _run(*args, "--dump-outputs", str(tmp_path / tag))
        assert all(k in rec for k in HEADLINE), rec.keys()
        assert rec["steps"] == 6 and rec["value"] > 0 and rec["ms_per_step"] > 0
        assert abs(rec["value"] - 256 * 250 * 6 / (rec["ms_per_step"] * 6 / 1e3)) < 1e-6 * rec["value"]
        assert not {"cpu_baseline", "extras", "clocks_mhz"} & set(rec), rec.keys()
        runs.append(_load(str(tmp_path / tag)))
    a, b = runs
    assert set(a) == set(b) and {"S_rz", "theta_rz", "column_index", "scalars"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    for k in a:
        assert a[k].dtype == np.float64, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    cols = a["column_index"]
    assert cols.size <= 256 * 250 and np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < 256 * 250
    assert a["S_rz"].shape == cols.shape and np.all(np.isfinite(a["S_rz"]))


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline():
    rec = _run("--gpus", "1", "--steps", "4", "--warmup", "2", "--size", "64", "50", "--cpu-cells", "2000", "--full")
    assert rec["steps"] == 4 and rec["cpu_baseline"]["value"] > 0 and "clocks_mhz" in rec


@pytest.mark.gpu
def test_sas_run_dumps_its_outputs(tmp_path):
    rec = _run("--model", "sas", "--size", "40", "25", "--ages", "100", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert rec["steps"] == 2 and "cpu_baseline" not in rec
    got = _load(str(tmp_path))
    assert got["sa_rz"].shape[0] == 1000 and got["C_iso_q_ss"].shape == (1000,)
    np.testing.assert_array_equal(got["column_index"], np.arange(1000))
