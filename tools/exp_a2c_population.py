"""Wall time of one iteration of a population of A2C learners (ppo.PopulationA2C) against the path the
project had for it: P separate A2C(fused_update=True, rollout_kernel="lanes") learners of 64 envs, each run with
learn(use_graph=True), one after the other.  P members of 64 envs, A2CConfig.reference() (RMSpropTFLike, eps 1e-9),
n_steps = 5, PID_LIKE / DIRECT_CONTROL at sample_time 0.05.

  separate     for every learner in turn: A2C.learn(--iters, use_graph=True) -- its env reset, --iters replays of its
               captured iteration, the statistics' host read after each (it is part of learn());
  population   PopulationA2C.learn(--iters): rollout, GAE, update and repack for all members, about six launches;
  pop_graph    PopulationA2C.learn(--iters, use_graph=True): the same as one graph replay per iteration.
Milliseconds per iteration OF THE WHOLE POPULATION (the time of the learn() calls / --iters).  Per member count one
process, the three cases alternating; medians of --runs rounds after a warm-up round (first launches, the captures),
torch.cuda.synchronize around every timed part; spread = max - min.  Every member count runs in a child process of its
own under a time limit of its own (--limit seconds), one after the other; the first that fails ends the run.
  python tools/exp_a2c_population.py [--out profiles/a2c_population.json] [--runs 7] [--iters 10]
                                     [--members 16 256 1024] [--limit 900]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, ST, TK, EPP = 5, 0.05, 20.0, 64


def summary(ts, scale=1e3):
    return {"median": scale * statistics.median(ts), "min": scale * min(ts), "max": scale * max(ts),
            "spread": scale * (max(ts) - min(ts))}


def env_of(n, offset=0):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=TK, sample_time=ST, seed=3,
                              env_offset=offset)


def measure(P, runs, iters):
    import torch
    from b747_rl_ctrl_amd.ppo import A2C, A2CConfig, PopulationA2C
    t0 = time.perf_counter()
    separate = [A2C(env_of(EPP, p * EPP), A2CConfig.reference(), seed=1 + p, fused_update=True, rollout_kernel="lanes")
                for p in range(P)]
    pops = {name: PopulationA2C(env_of(P * EPP), P, EPP, A2CConfig.reference(), seeds=[1 + p for p in range(P)], seed=1)
            for name in ("population", "pop_graph")}
    torch.cuda.synchronize()
    built = time.perf_counter() - t0

    def run(name):
        if name == "separate":
            for a2c in separate:
                a2c.learn(iters, use_graph=True)
        else:
            pops[name].learn(iters, use_graph=name == "pop_graph")

    ts = {"separate": [], "population": [], "pop_graph": []}
    for r in range(runs + 1):                   # round 0: the warm-up (and the captures)
        for name in ts:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name)
            torch.cuda.synchronize()
            if r:
                ts[name].append((time.perf_counter() - t0) / iters)
    out = {k: summary(v) for k, v in ts.items()}
    out["unit"] = "ms per iteration of all members"
    out["separate_over_pop_graph"] = out["separate"]["median"] / out["pop_graph"]["median"]
    out["separate_over_population"] = out["separate"]["median"] / out["population"]["median"]
    out["build_seconds"] = built
    n_params = pops["population"].n_params
    out["finite"] = all(bool(torch.isfinite(pp.flat[:, :n_params]).all()) for pp in pops.values()) and \
        all(bool(torch.isfinite(a2c.flat[:n_params]).all()) for a2c in separate)
    out["steps_taken"] = [int(pp.upd_t[0]) for pp in pops.values()] + [int(separate[0].upd_t)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2c_population.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--members", type=int, nargs="*", default=[16, 256, 1024])
    ap.add_argument("--limit", type=float, default=900.0, help="seconds one member count may take")
    ap.add_argument("--case", type=int, default=0, help="(child) measure this member count, one JSON line")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.case:
        import torch
        res = measure(a.case, a.runs, a.iters)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        return
    res = {"what": __doc__.split("\n  python")[0], "command": "python tools/exp_a2c_population.py " + " ".join(sys.argv[1:]),
           "n_steps": T, "envs_per_member": EPP, "config": "A2CConfig.reference()", "runs": a.runs, "iters": a.iters,
           "members": {}}
    for P in a.members:                         # (the parent never opens the GPU: one process with it at a time)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(P), "--runs", str(a.runs),
                                "--iters", str(a.iters)], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            res["members"][str(P)] = {"error": f"no result within {a.limit:.0f} s"}
            print("members", P, "timed out", flush=True)
            break
        if r.returncode != 0:
            res["members"][str(P)] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            print("members", P, "failed", r.returncode, r.stderr[-2000:], flush=True)
            break
        res["members"][str(P)] = json.loads(r.stdout.strip().splitlines()[-1])
        res["device"] = res["members"][str(P)].pop("device")
        print("members", P, json.dumps(res["members"][str(P)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if any("error" in v for v in res["members"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
