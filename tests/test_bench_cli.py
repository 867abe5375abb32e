"""bench.py's command line: what a plain run prints, what --dump-outputs writes (the state a caller of the timed path holds after the last timed
step), and the byte budget of that dump."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

# what only --full adds to the result line
FULL_ONLY = ("factorisation", "roofline", "cpu_baseline", "several_filters_one_gpu", "frame_mix", "reference_side_binding", "other_state_sizes")


class _FakeFilter:
    def __init__(self, N, seed=0):
        rng = np.random.default_rng(seed)
        self.sensor, self.ids, self.p = rng.normal(size=23), np.arange(7, 7 + N, dtype=np.int32), rng.normal(size=(N, 3))
        A = rng.normal(size=(21 + 3 * N, 21 + 3 * N))
        self.S = np.asfortranarray(A @ A.T)

    def state_estimate(self):
        return self.sensor, self.ids, self.p

    def get_sigma(self):
        return self.S


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_state_estimate_and_sigma_in_float64(tmp_path):
    flt = _FakeFilter(10)
    bench.dump_outputs(flt, str(tmp_path / "out"))
    got = _load(str(tmp_path / "out"))
    assert sorted(got) == ["landmark_ids", "landmark_positions", "sensor_state", "sigma"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["sensor_state"], flt.sensor) and np.array_equal(got["landmark_positions"], flt.p)
    assert np.array_equal(got["landmark_ids"], flt.ids.astype(np.float64)) and np.array_equal(got["sigma"], flt.S)


def test_dump_outputs_samples_a_sigma_beyond_the_budget_the_same_way_every_time(tmp_path):
    flt = _FakeFilter(30)
    budget = 16384
    for d in ("a", "b"):
        bench.dump_outputs(flt, str(tmp_path / d), budget=budget)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert "sigma" not in a and sum(v.nbytes for v in a.values()) <= budget
    idx = a["sigma_sample_index"].astype(np.int64)
    assert len(idx) > 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["sigma_sample"], flt.S.ravel(order="F")[idx])
    assert all(np.array_equal(a[k], b[k]) for k in a)  # a fixed, seeded sample


def test_bench_refuses_zero_steps():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "--steps" in res.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only_and_dumps_the_timed_steps_outputs(tmp_path):
    N, steps, warmup = 50, 30, 5
    out_dir = str(tmp_path / "outputs")
    env = dict(os.environ, EQVIO_BENCH_SPIN_UP_S="0.05")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--landmarks", str(N), "--dump-outputs", out_dir]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    d = json.loads(lines[-1])
    assert d["unit"] == "updates/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-9)
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    got = _load(out_dir)
    assert sorted(got) == ["landmark_ids", "landmark_positions", "sensor_state", "sigma"]
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
    S = got["sigma"]
    assert S.shape == (21 + 3 * N, 21 + 3 * N) and np.all(np.diag(S) > 0)
    _, frames = bench.build_workload(seed=100, n_frames=warmup + steps + 2, N=N)  # rank 0's world, as the run built it
    assert got["landmark_positions"].shape == (N, 3) and sorted(got["landmark_ids"].astype(int).tolist()) == sorted(frames[warmup + steps - 1][2].tolist())
