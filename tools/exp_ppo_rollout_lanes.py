"""PPO.collect_rollouts through the one-wave rollout kernel (rollout_kernel="lanes", b747_ppo_rollout_lanes: two
launches per rollout) against the parent's path for the same envs (rollout_kernel=False with use_graph=True: two
launches per step, replayed as one graph), DESIGN.md 12.  The two paths alternate in one process, medians of `--rounds`
after a warm-up of each (the warm-up holds the graph captures), torch.cuda.synchronize around every timed call.
  configurations  PID_LIKE / ADD_DIRECT / CONST and SPEED_MODE / ADD_PROC / HYBRID (main.py's settings, tk = 20, no
                  disturbance), at sample_time 0.05 and 0.01
  shapes          65,536 envs x 64 steps, 4,096 x 64 and 4 x 2,048 (SB3's default shape)
  orientation     the bench configuration (PID_LIKE / DIRECT / CONST / AERO, sample_time 0.05) at 65,536 x 64 with
                  b747_ppo_rollout's two-wave kernel (rollout_kernel=True) beside the two
The baseline is always the parent's path, never the code under test.
--variants tag=lib.so,...: the "lanes" time of A/B builds of the library (e.g. -DB747_LANES_SKIP_VALUE: the kernel
without its value head), each in a child process of its own (B747_LIB_PATH), at the three shapes, sample_time 0.05.
Run: python tools/exp_ppo_rollout_lanes.py [--out profiles/ppo_rollout_lanes.json] [--rounds 5] [--variants t=x.so,...]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_rollout_lanes.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--variants", default="", help="tag=path,... A/B libraries for the lanes-only sweep")
ap.add_argument("--lanes-only", action="store_true", help="the lanes times of the loaded library as one JSON line")
a = ap.parse_args()

SHAPES = [(65536, 64), (4096, 64), (4, 2048)]            # (envs, steps)
SAMPLE_TIMES = (0.05, 0.01)
CONFIGS = {"PID_LIKE/ADD_DIRECT/CONST": ("PID_LIKE", "ADD_DIRECT_CONTROL", "CONST"),
           "SPEED_MODE/ADD_PROC/HYBRID": ("SPEED_MODE", "ADD_PROC_CONTROL", "HYBRID")}

sweep = {}
if a.variants and not a.lanes_only:                      # children first: one process with the GPU open at a time
    for spec in [("product", "")] + [tuple(s.split("=", 1)) for s in a.variants.split(",")]:
        env = dict(os.environ)
        if spec[1]:
            env["B747_LIB_PATH"] = os.path.abspath(spec[1])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lanes-only", "--rounds", str(a.rounds)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"variant {spec[0]} failed ({r.returncode}):\n{r.stderr[-2000:]}")
        sweep[spec[0]] = json.loads(r.stdout.strip().splitlines()[-1])

import torch  # noqa: E402

from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, DisturbanceMode, ObservationType,  # noqa: E402
                              ResetRefMode, RewardType)
from b747_rl_ctrl_amd.ppo import PPO, PPOConfig  # noqa: E402

dev = torch.device("cuda")
ACTION_MAX = {"DIRECT_CONTROL": 17 * math.pi / 180, "ADD_PROC_CONTROL": 1.0,
              "ADD_DIRECT_CONTROL": 10 * math.pi / 180}   # main.py:7-12


def make_env(n, obs, mode, reset, sample_time, aero=False):
    return BatchControllerEnv(n, ObservationType[obs], RewardType.CLASSIC, True, True, CtrlType.MANUAL, CtrlMode[mode],
                              reset_ref_mode=ResetRefMode[reset],
                              disturbance_mode=DisturbanceMode.AERO_DISTURBANCE if aero else None, tk=20,
                              sample_time=sample_time, action_max=ACTION_MAX[mode], seed=98, device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def race(paths, T):
    """paths: name -> PPO.  Alternated, round 0 the warm-up (graph captures); seconds per collect_rollouts"""
    ts = {k: [] for k in paths}
    for rnd in range(a.rounds + 1):
        for name, ppo in paths.items():
            dt = timed(lambda: ppo.collect_rollouts(T, use_graph=True))
            if rnd:
                ts[name].append(dt)
    return ts


def summary(ts, envs, T):
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"envs": envs, "steps": T,
            "collect_rollouts_ms": {k: {"median": round(1e3 * med[k], 3), "spread": round(1e3 * (max(v) - min(v)), 3),
                                        "all": [round(1e3 * x, 3) for x in v]} for k, v in ts.items()},
            "us_per_step": {k: round(1e6 * v / T, 2) for k, v in med.items()},
            "env_steps_per_second": {k: round(envs * T / v) for k, v in med.items()}}


def paths_for(envs, T, obs, mode, reset, st, aero=False, split=False):
    kinds = {"lanes": "lanes", "two_launch_graph": False}
    if split:
        kinds["split_kernel"] = True
    if a.lanes_only:
        kinds = {"lanes": "lanes"}
    out = {}
    for name, kind in kinds.items():
        env = make_env(envs, obs, mode, reset, st, aero)
        ppo = PPO(env, PPOConfig(n_steps=T, batch_size=65536), seed=0, rollout_kernel=kind)
        ppo.last_obs.copy_(env.obs)
        out[name] = ppo
    return out


if a.lanes_only:
    res = {}
    for label, (obs, mode, reset) in CONFIGS.items():
        for envs, T in SHAPES:
            ts = race(paths_for(envs, T, obs, mode, reset, 0.05), T)["lanes"]
            res[f"{label} {envs}x{T}"] = {"ms_median": round(1e3 * statistics.median(ts), 3),
                                          "ms_spread": round(1e3 * (max(ts) - min(ts)), 3)}
            torch.cuda.empty_cache()
    print(json.dumps(res))
    sys.exit(0)

table = {}
for label, (obs, mode, reset) in CONFIGS.items():
    for st in SAMPLE_TIMES:
        for envs, T in SHAPES:
            paths = paths_for(envs, T, obs, mode, reset, st)
            row = summary(race(paths, T), envs, T)
            m = row["collect_rollouts_ms"]
            row["sample_time"] = st
            row["launches_per_rollout"] = {"lanes": 2, "two_launch_graph": 2 * T}
            row["ratio_two_launch_over_lanes"] = round(m["two_launch_graph"]["median"] / m["lanes"]["median"], 3)
            row["lanes_faster_beyond_the_spread"] = bool(m["two_launch_graph"]["median"] - m["lanes"]["median"]
                                                         > m["two_launch_graph"]["spread"] + m["lanes"]["spread"])
            table[f"{label} st={st} {envs}x{T}"] = row
            print(f"{label} st={st} {envs}x{T}: {row['collect_rollouts_ms']}", file=sys.stderr, flush=True)
            del paths
            torch.cuda.empty_cache()

envs, T = SHAPES[0]
paths = paths_for(envs, T, "PID_LIKE", "DIRECT_CONTROL", "CONST", 0.05, aero=True, split=True)
assert paths["split_kernel"].rollout_kernel is True
bench_row = summary(race(paths, T), envs, T)
bench_row["sample_time"] = 0.05
del paths

try:
    import kernel_resources
    lib = os.environ.get("B747_LIB_PATH") or os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
    resources = {n: f for n, f in kernel_resources.resources(lib).items() if "k_rollout_lanes<" in n}
except Exception as e:  # the LLVM tools are missing: the timings stand without the figures
    resources = {"error": repr(e)}

out = {
    "what": "PPO.collect_rollouts(use_graph=True): rollout_kernel=\"lanes\" (b747_ppo_rollout_lanes) against the parent's "
            "path for these envs (rollout_kernel=False: b747_policy_act + b747_env_rollout(K = 1) per step, one graph), "
            "alternated in one process, medians over the rounds after a warm-up",
    "rounds": a.rounds,
    "rollouts": table,
    "bench_configuration_65536x64": bench_row,
    "lanes_variants_ms": sweep or None,
    "kernel_resources": resources,
    "device": torch.cuda.get_device_name(0),
}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
