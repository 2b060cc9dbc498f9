"""Wall time of an A2C iteration (ppo.A2C) with the torch update, with the fused update
(b747_a2c_update), and with the fused update inside one HIP graph per iteration, and of the update alone.  SB3's
n_steps = 5 at 4,096 and 65,536 envs (20,480 and 327,680 rows per step), the reference's entry (A2CConfig.reference():
RMSpropTFLike, eps 1e-9), PID_LIKE / DIRECT_CONTROL at sample_time 0.05, the one-wave rollout kernel
(rollout_kernel="lanes").

  iteration   A2C.learn(--iters) per case, alternating: "torch" (fused_update=False), "fused" (fused_update=True),
              "fused_graph" (fused_update=True, use_graph=True); milliseconds per iteration, the statistics' host read
              included (it is part of learn()).
  update      A2C._update(T) alone on the rollout the learner holds -- the step, the modules brought up to date and the
              repack -- "torch" against "fused", alternating; milliseconds per update.
One process, one GPU; medians of --runs after a warm-up round (first launches, the capture), torch.cuda.synchronize around
every timed part; spread = max - min.
  python tools/exp_a2c.py [--out profiles/a2c.json] [--runs 7] [--iters 20] [--envs 4096 65536]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, ST, TK = 5, 0.05, 20.0


def summary(ts, scale=1e3):
    return {"median": scale * statistics.median(ts), "min": scale * min(ts), "max": scale * max(ts),
            "spread": scale * (max(ts) - min(ts))}


def learner(n, fused_update):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    from b747_rl_ctrl_amd.ppo import A2C, A2CConfig
    env = BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=TK, sample_time=ST, seed=3)
    return A2C(env, A2CConfig.reference(), seed=1, fused_update=fused_update, rollout_kernel="lanes")


def measure(n, runs, iters):
    import torch
    cases = {"torch": (learner(n, False), False), "fused": (learner(n, True), False),
             "fused_graph": (learner(n, True), True)}
    ts = {k: [] for k in cases}
    for r in range(runs + 1):                   # round 0: the warm-up (and the capture)
        for name, (a2c, graph) in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a2c.learn(iters, use_graph=graph)
            torch.cuda.synchronize()
            if r:
                ts[name].append((time.perf_counter() - t0) / iters)
    out = {"iteration": {k: summary(v) for k, v in ts.items()}}
    out["iteration"]["unit"] = "ms per iteration"
    out["rollout_kernel"] = str(cases["fused"][0].rollout_kernel)
    ts = {"torch": [], "fused": []}
    for r in range(runs + 1):
        for name in ts:
            a2c = cases[name][0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                a2c._update(T)
            torch.cuda.synchronize()
            if r:
                ts[name].append((time.perf_counter() - t0) / iters)
    out["update"] = {k: summary(v) for k, v in ts.items()}
    out["update"]["unit"] = "ms per update"
    out["finite"] = all(bool(torch.isfinite(a2c.flat[:sum(p.numel() for p in a2c.policy.flat_param_list())]).all())
                        for a2c, _ in cases.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2c.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 65536])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    res = {"what": __doc__.split("\n  python")[0], "command": "python tools/exp_a2c.py " + " ".join(sys.argv[1:]),
           "n_steps": T, "config": "A2CConfig.reference()", "runs": a.runs, "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "envs": {}}
    for n in a.envs:
        res["envs"][str(n)] = measure(n, a.runs, a.iters)
        print("envs", n, json.dumps(res["envs"][str(n)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
