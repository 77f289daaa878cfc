"""bench.py's command line: a plain run (--gpus 1 --steps K --warmup W) times K steps and prints
the headline line only; --dump-outputs DIR writes what the last timed step returned, the same
from run to run; --full adds the legs, the CPU baseline and the quoted profiles."""
import json

import numpy as np
import pytest

import bench

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("primitive_fingertips", "capsule_hand", "unrefined_solve", "cpu_baseline", "valu_roofline", "qpos_drift")
DUMPED = {"obs": 2, "reward": 1, "discount": 1, "step_type": 1, "qpos": 2, "qvel": 2}  # name -> ndim


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path):
    rng = np.random.RandomState(0)
    arrays = {"obs": rng.rand(100, 7), "step_type": rng.randint(0, 3, 100).astype(np.uint8)}
    bench.dump_outputs(tmp_path / "whole", arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "whole").glob("*.npy")}
    assert set(got) == set(arrays) and all(v.dtype == np.float32 for v in got.values())
    np.testing.assert_array_equal(got["obs"], arrays["obs"].astype(np.float32))
    np.testing.assert_array_equal(got["step_type"], arrays["step_type"])
    # 100 envs x (7 + 1 floats + the index) = 4000 B: a budget of 1000 B keeps 25 envs, the same ones twice
    for d in ("s1", "s2"):
        bench.dump_outputs(tmp_path / d, arrays, budget=1000)
    s1 = {p.stem: np.load(p) for p in (tmp_path / "s1").glob("*.npy")}
    rows = s1["env_index"].astype(int)
    assert len(rows) == 25 and len(set(rows)) == 25 and (np.diff(rows) > 0).all() and s1["env_index"].dtype == np.float64
    assert sum(v.nbytes for v in s1.values()) <= 1000
    np.testing.assert_array_equal(s1["obs"], arrays["obs"][rows].astype(np.float32))
    np.testing.assert_array_equal(s1["step_type"], arrays["step_type"][rows])
    for p in (tmp_path / "s1").glob("*.npy"):
        np.testing.assert_array_equal(np.load(tmp_path / "s2" / p.name), s1[p.stem])


def _run(capsys, *argv):
    bench.main(["--gpus", "1", *argv])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1  # ONE result line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(capsys, tmp_path):
    """Two plain runs with the same arguments: the headline keys and nothing that takes a run of
    its own; the dumped arrays (float32, one row per env, finite) are equal bit for bit."""
    argv = ("--envs", "96", "--steps", "3", "--warmup", "2")
    lines = [_run(capsys, *argv, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "env-steps/s" and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(96 * 1e3 / line["ms_per_step"])
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(a) == set(DUMPED)
    for k, v in a.items():
        assert v.dtype == np.float32 and v.ndim == DUMPED[k] and v.shape[0] == 96 and np.isfinite(v).all(), k
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{k}.npy"), v)
    assert np.abs(a["qvel"]).max() > 0 and np.abs(a["obs"]).max() > 0  # stepped, not the reset state
    assert set(np.unique(a["step_type"])) <= {0.0, 1.0, 2.0}


@pytest.mark.gpu
def test_full_run_keeps_what_moved(capsys):
    """--full: the legs, the CPU baseline, the logged returns and the profiles' entries are on the line."""
    line = _run(capsys, "--full", "--envs", "96", "--steps", "2", "--warmup", "1", "--cpu-sample-envs", "2",
                "--cpu-sample-steps", "5")
    assert all(k in line for k in HEADLINE + FULL_ONLY)
    for leg in ("primitive_fingertips", "capsule_hand", "unrefined_solve"):
        assert line[leg]["value"] > 0 and line[leg]["ms_per_step"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert {"mean_return_logged", "episodes_finished", "solver_last_step"} <= set(line["config"])
    assert {"traffic", "wave_time"} <= set(line["roofline"])
