"""bench.py's plain run and its --dump-outputs: a plain run times exactly --steps sweeps and prints
the headline line only (the secondary measurements are behind --full); the dumped iterates are
float64 .npy files, and two runs with the same arguments write the same values (the inputs are
generated from a fixed seed on the device, the sweep's reductions run in a fixed order)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from epsilon_amd import problems, wire  # noqa: E402


def _status(**res):
    return wire.SolverStatus(state=2, residuals=wire.Residuals(**res)).SerializeToString()


def test_dump_outputs_writes_every_variable_and_the_residuals(tmp_path):
    x = np.arange(5, dtype=np.float64)
    y = -np.arange(5, dtype=np.float64)
    xs = {problems.LASSO_COPY: x.tobytes(), problems.LASSO_VAR: y.tobytes()}
    bench.dump_outputs(str(tmp_path), _status(r_norm=1.5, s_norm=2.5, epsilon_primal=0.1, epsilon_dual=0.2), xs)
    assert sorted(os.listdir(tmp_path)) == ["residuals.npy", "separate_var_x_sum_square.npy", "var_x.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "var_x.npy"), y)
    np.testing.assert_array_equal(np.load(tmp_path / "separate_var_x_sum_square.npy"), x)
    r = np.load(tmp_path / "residuals.npy")
    assert r.dtype == np.float64
    np.testing.assert_array_equal(r, [1.5, 2.5, 0.1, 0.2])


def test_dump_outputs_takes_a_fixed_sample_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 1000)
    x = np.random.RandomState(1).randn(4000)
    xs = {"var:a": x.tobytes(), "var:b": (2 * x).tobytes()}
    bench.dump_outputs(str(tmp_path / "one"), _status(r_norm=1.0), xs)
    bench.dump_outputs(str(tmp_path / "two"), _status(r_norm=1.0), xs)
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= 8 * 1000 + 4 * 128  # the limit plus the .npy headers
    idx = np.load(tmp_path / "one" / "sample_index.npy").astype(np.int64)
    assert idx.size > 0 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "one" / "var_a.npy"), x[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "one" / "var_b.npy"), 2 * x[idx])
    for f in os.listdir(tmp_path / "one"):
        np.testing.assert_array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f))


def _plain_run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
           "--dump-outputs", out_dir]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    one = _plain_run(str(tmp_path / "one"), 7)
    two = _plain_run(str(tmp_path / "two"), 7)
    for line in (one, two):
        assert line["steps"] == 7 and line["warmup"] == 3
        assert line["unit"] == "iter/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
        # the secondary measurements are --full only
        for k in ("time_to_eps_s", "iters_to_eps", "roofline", "kernels", "cpu_baseline"):
            assert k not in line, k
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == sorted(os.listdir(tmp_path / "two"))
    assert "var_x.npy" in files and "residuals.npy" in files
    for f in files:
        a, b = np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f)
        assert a.dtype == np.float64 and np.all(np.isfinite(a)), f
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert np.load(tmp_path / "one" / "var_x.npy").shape == (50000,)
