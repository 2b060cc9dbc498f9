"""Wall time of PopulationPPO's train() and of a whole learn() iteration with the sample orders drawn on the host
(sample_order="host", the default: per member a torch.randperm, then a stack and a gather), on the device
(sample_order="device": one b747_ppo_sample_orders launch per epoch) and on the device with the iteration replayed as
one HIP graph (learn(use_graph=True)); DESIGN.md 18.  P members of 64 envs for P in --members, T = 64 (4,096 rows per
member), batch_size 1,024, n_epochs 10, batched_update=True.  One process, one GPU; the paths alternate round by round;
medians of --runs after a warm-up round (which also captures the graph), torch.cuda.synchronize around every timed
part; spread = max - min.
  iteration: learn(1, T[, use_graph=True]) -- the env reset, the rollout, GAE, train and the statistics;
  train:     train(T) after a rollout and compute_gae of its own (not separable from a replayed iteration).
--paths host also runs on a tree from before sample_order (the baseline of the default path: --root that tree).
  python tools/exp_ppo_sample_order.py [--out profiles/ppo_sample_order.json] [--runs 5] [--members 16 64 256]
                                       [--paths host device device_graph] [--root DIR]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPP, T, BATCH, EPOCHS, ST, TK = 64, 64, 1024, 10, 0.05, 20.0
SEED = 1
PATHS = ("host", "device", "device_graph")


def summary(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts),
            "spread_ms": 1e3 * (max(ts) - min(ts))}


def population(P, path):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    env = BatchControllerEnv(P * EPP, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=TK, sample_time=ST, seed=3)
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS)
    kw = {} if path == "host" else {"sample_order": "device"}      # (no keyword on the default path: any tree runs it)
    return PopulationPPO(env, P, EPP, cfg, seed=SEED, batched_update=True,
                         learning_rates=[3e-4 * (1 + (p % 5) * 0.5) for p in range(P)], **kw)


def measure(P, paths, runs):
    import torch
    pops = {path: population(P, path) for path in paths}
    ts = {path: {"iteration": [], "train": []} for path in paths}
    for r in range(runs + 1):                   # round 0: the warm-up (and the capture)
        for path, pp in pops.items():           # alternated
            kw = {"use_graph": True} if path == "device_graph" else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pp.learn(1, T, **kw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r:
                ts[path]["iteration"].append(t1 - t0)
            if path == "device_graph":
                continue
            pp.collect_rollouts(T)
            pp.compute_gae(T)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pp.train(T)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r:
                ts[path]["train"].append(t1 - t0)
    out = {path: {part: summary(v) for part, v in parts.items() if v} for path, parts in ts.items()}
    # (the paths run different numbers of rollouts between their timed parts, so their parameters differ by now: parity
    # is the test suite's, tests/test_gpu_ppo_population_device_order_train.py; here only that everyone still trains)
    out["finite"] = all(bool(torch.isfinite(pp.flat[:, :pp.n_params]).all()) for pp in pops.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_sample_order.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--members", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--paths", nargs="+", default=list(PATHS), choices=PATHS)
    ap.add_argument("--root", default=ROOT, help="the tree whose b747_rl_ctrl_amd to measure")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import b747_rl_ctrl_amd
    print("measuring", os.path.dirname(os.path.abspath(b747_rl_ctrl_amd.__file__)), flush=True)
    res = {"what": __doc__.split("\n  python")[0], "envs_per_member": EPP, "T": T, "batch_size": BATCH,
           "n_epochs": EPOCHS, "runs": a.runs, "paths": a.paths, "device": torch.cuda.get_device_name(0), "members": {}}
    for P in a.members:
        res["members"][str(P)] = measure(P, a.paths, a.runs)
        print(P, json.dumps(res["members"][str(P)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
