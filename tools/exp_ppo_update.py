"""PPO.train at the bench's training shape (65,536 envs x 64 steps, minibatches of 65,536, 10 epochs = 640
minibatch steps): the default torch update against fused_update=True (b747_ppo_grad + b747_ppo_adam), alternated in
one process on one rollout shape, medians of `--rounds` after a warm-up of each.  bench.py's ppo_training line keeps
measuring the default path; this is the figure for the fused one.
Run: python tools/exp_ppo_update.py [--out profiles/ppo_update.json] [--rounds 5] [--envs 65536]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from b747_rl_ctrl_amd.ppo import PPO, PPOConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--only", choices=["default", "fused"], help="one path alone, no file written (for a profiler run)")
a = ap.parse_args()

dev = torch.device("cuda")
paths = {}
for name in ("default", "fused"):
    if a.only and a.only != name:
        continue
    env = bench.make_env(a.envs, 0, True, dev, seed=98, sample_time=0.05)
    ppo = PPO(env, PPOConfig(n_steps=a.steps, batch_size=65536), seed=0, fused_update=(name == "fused"))
    ppo.last_obs.copy_(env.obs)
    ppo.collect_rollouts(a.steps)
    ppo.compute_gae(a.steps)
    paths[name] = ppo


def timed_train(ppo):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = ppo.train(a.steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, stats


times = {name: [] for name in paths}
last = {}
for rnd in range(a.rounds + 1):                # round 0: the warm-up (allocator, kernel loading), not counted
    for name, ppo in paths.items():
        dt, last[name] = timed_train(ppo)
        if rnd:
            times[name].append(dt)
if a.only:
    print(json.dumps({a.only: times[a.only]}))
    sys.exit(0)

n_mb = paths["fused"].cfg.n_epochs * -(-a.envs * a.steps // paths["fused"].cfg.batch_size)
med = {name: statistics.median(t) for name, t in times.items()}
spread = {name: max(t) - min(t) for name, t in times.items()}
out = {
    "what": "PPO.train seconds, default (torch) and fused_update paths alternated in one process, medians",
    "envs": a.envs, "rollout_steps": a.steps, "batch_size": 65536, "epochs": paths["fused"].cfg.n_epochs,
    "minibatch_steps": n_mb, "rounds": a.rounds,
    "train_seconds": {k: [round(x, 5) for x in v] for k, v in times.items()},
    "median_seconds": {k: round(v, 5) for k, v in med.items()},
    "spread_seconds": {k: round(v, 5) for k, v in spread.items()},
    "us_per_minibatch": {k: round(1e6 * v / n_mb, 2) for k, v in med.items()},
    "ratio_default_over_fused": round(med["default"] / med["fused"], 2),
    "faster_by_more_than_the_spread": bool(med["default"] - med["fused"] > spread["default"] + spread["fused"]),
    "last_stats": {k: {s: v[s] for s in ("loss", "value_loss", "policy_gradient_loss", "approx_kl", "clip_fraction")}
                   for k, v in last.items()},
    "note": "bench.py's ppo_training line measures the default path; it is not changed by fused_update",
    "device": torch.cuda.get_device_name(0),
}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
