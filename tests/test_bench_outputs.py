"""bench.py's plain run and --dump-outputs: a plain run measures the headline only (what needs a run of its own is
null until --full), --steps sets the timed steps, and the last timed step's outputs are written as <name>.npy in
float32 / float64, identical from run to run for the same arguments."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ["done", "episode_length", "episode_return", "obs", "reward", "terminal_observation"]


def test_dump_writes_float_arrays_and_samples_past_the_cap(tmp_path, monkeypatch):
    torch = bench.torch
    n = 1000
    out = {"obs": torch.arange(3 * n, dtype=torch.float32).reshape(n, 3), "reward": torch.arange(n, dtype=torch.float64),
           "done": torch.arange(n) % 2 == 0, "episode_length": torch.arange(n, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "a"), out, 0)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["done", "episode_length", "obs", "reward"]
    assert got["reward"].dtype == np.float64 and all(got[k].dtype == np.float32 for k in ("obs", "done", "episode_length"))
    assert all(np.array_equal(got[k], out[k].numpy().astype(got[k].dtype)) for k in got)
    # past the cap: the same fixed rows of every array, named by rows.npy, within the cap, the same on every call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), out, 0)
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    rows = b["rows"].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and sum(a.nbytes for a in b.values()) <= 4096
    assert all(np.array_equal(b[k], got[k][rows]) for k in got)
    assert all(np.array_equal(b[k], np.load(tmp_path / "c" / (k + ".npy"))) for k in b)
    bench.dump_outputs(str(tmp_path / "b"), out, 1)
    assert os.path.exists(tmp_path / "b" / "obs.rank1.npy")


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_every_run(tmp_path, monkeypatch, capsys):
    n, args = 1000, ("--envs", "1000", "--steps", "7", "--warmup", "3")
    d = [_run(monkeypatch, capsys, *args, "--dump-outputs", str(tmp_path / t)) for t in "ab"][0]
    assert d["metric"] == "env steps/sec (batched B747 pitch sim)" and d["unit"] == "env-steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 7 and d["warmup"] == 3
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-2)
    # nothing that takes a run of its own
    for k in ("rollout", "ppo_rollout", "storage_f32", "sample_time_0.05", "ppo_training", "variant_mixed", "config2"):
        assert d[k] is None, k
    assert "cpu_baseline" not in d and "cpu_baseline_batched" not in d
    assert d["roofline"]["isolated_launch_us"] is None and d["roofline"]["replays_after_us_per_step"] is None
    assert d["roofline"]["kernel_avg_us"] > 0
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == NAMES
    assert a["obs"].shape == (n, 3) and a["terminal_observation"].shape == (n, 3)
    assert all(a[k].shape == (n,) for k in ("reward", "done", "episode_return", "episode_length"))
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert np.abs(a["obs"]).max() > 0 and set(np.unique(a["done"])) <= {0.0, 1.0}
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k
    # the outputs are the last TIMED step's: more steps of its own afterwards (--full) leave them as they are
    f = _run(monkeypatch, capsys, *args, "--full", "--no-rollout", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "f"))
    assert f["roofline"]["isolated_launch_us"] > 0 and len(f["roofline"]["replays_after_us_per_step"]) == 2
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "f" / (k + ".npy"))), k
