"""Wall time of the population evaluation (b747_eval_population) against the path the library had
before it, in one process on one GPU:
  policies  evaluate.population_step_tests with P policies (one launch) against P sequential
            evaluate.run_step_tests_fused calls (one launch, one env batch and one pack each);
  gains     evaluate.pid_sweep_step_tests with G gain sets x 4 references (one launch) against G sequential launches
            with the gain set in the batch's consts (agent_test.set_pid_coefs + eval_episodes, one env batch each);
  kernel    at 65,536 envs, alternated call by call: b747_eval_episodes, b747_eval_population with one policy and no
            gains, and b747_eval_population with one policy and every env's own (default) SS gains -- the cost of the
            population form where it is not needed, and of the per-lane gains.
Above 16 sequential calls only 16 are timed and the figure is scaled to P (or G): "extrapolated": true says so.
tk 20 s, sample_time 0.05 (400 env steps, 2,000 DLL steps).  Medians of --runs after a warm-up, torch.cuda.synchronize
around every timed call.
  python tools/exp_eval_population.py [--out profiles/eval_population.json] [--runs 5]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

REFS = [5 * math.pi / 180, -5 * math.pi / 180, 10 * math.pi / 180, -10 * math.pi / 180]
TK, ST = 20.0, 0.05
SEQ_MAX = 16


def measure(fn, runs):
    fn()                                          # warm-up (module loads, allocator)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        del out
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def scaled(m, factor, count):
    out = {k: v * factor for k, v in m.items()}
    out["calls_timed"] = count
    out["extrapolated"] = factor != 1.0
    return out


def verdict(one, seq):
    """faster by more than both spreads?"""
    spread = lambda m: m["max_s"] - m["min_s"]
    return {"speedup": seq["median_s"] / one["median_s"],
            "beyond_both_spreads": seq["median_s"] - one["median_s"] > spread(one) + spread(seq)}


def policies_leg(runs):
    from b747_rl_ctrl_amd.evaluate import population_step_tests, run_step_tests_fused
    from b747_rl_ctrl_amd.ppo import ActorCritic
    torch.manual_seed(0)
    nets = [ActorCritic(3) for _ in range(SEQ_MAX)]
    base = torch.stack([n.flat_params().detach() for n in nets])
    kw = dict(tk=TK, sample_time=ST)
    out = {}
    for P in (1, 16, 256, 1024):
        flat = base[torch.arange(P) % SEQ_MAX] + 1e-3 * torch.randn(P, base.shape[1])
        k = min(P, SEQ_MAX)
        row = {"population": measure(lambda: population_step_tests(flat, REFS, **kw), runs),
               "sequential": scaled(measure(lambda: [run_step_tests_fused(n, REFS, **kw) for n in nets[:k]], runs),
                                    P / k, k)}
        row.update(verdict(row["population"], row["sequential"]))
        out[str(P)] = row
        print("policies", P, json.dumps(row), flush=True)
    return out


def gains_leg(runs):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlType, ObservationType, RewardType, _lib
    from b747_rl_ctrl_amd.agent_test import set_pid_coefs
    from b747_rl_ctrl_amd.evaluate import pid_sweep_step_tests
    default = torch.tensor(list(_lib.default_consts().PID_SS), dtype=torch.float64)
    kw = dict(tk=TK, sample_time=ST)

    def consts_sweep(gs):
        """run_step_tests_fused's env and launch per gain set, the gains in the batch's consts"""
        res = []
        for g in gs:
            env = BatchControllerEnv(len(REFS), ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.AUTO,
                                     None, reset_ref_mode=None, tk=TK, sample_time=ST, auto_reset=False)
            env.set_state0(torch.tensor([0, 11000, 250, 0, 0, 0], dtype=torch.float64))
            env.set_reference(vartheta=torch.tensor(REFS, dtype=torch.float64))
            set_pid_coefs(env, g.tolist())
            env.reset()
            res.append(env.eval_episodes(int(math.ceil(TK / ST - 1e-9)), None, "state_vartheta", scale=180 / math.pi,
                                         y_base=env.ref[0] * 180 / math.pi))
        return res

    out = {}
    gen = torch.Generator().manual_seed(1)
    for G in (16, 1024, 16384):
        gains = default[None] * (0.5 + torch.rand(G, 4, generator=gen, dtype=torch.float64))
        k = min(G, SEQ_MAX)
        row = {"envs": G * len(REFS),
               "sweep": measure(lambda: pid_sweep_step_tests(gains, REFS, "SS", **kw), runs),
               "sequential": scaled(measure(lambda: consts_sweep(gains[:k]), runs), G / k, k)}
        row.update(verdict(row["sweep"], row["sequential"]))
        out[str(G * len(REFS))] = row
        print("gains", G, json.dumps(row), flush=True)
    return out


def kernel_leg(runs, n=65536):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, RewardType, _lib
    from b747_rl_ctrl_amd.evaluate import pack_policies
    from b747_rl_ctrl_amd.ppo import ActorCritic
    torch.manual_seed(0)
    net = ActorCritic(3)
    env = BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=None, tk=TK, sample_time=ST, auto_reset=False)
    env.set_state0(torch.tensor([0, 11000, 250, 0, 0, 0], dtype=torch.float64))
    env.set_reference(vartheta=torch.tensor(REFS * (n // 4), dtype=torch.float64))
    packed = pack_policies([net], 3, env.device)
    gains = torch.tensor(list(_lib.default_consts().PID_SS), dtype=torch.float64, device=env.device).expand(n, 4)
    steps = int(math.ceil(TK / ST - 1e-9))
    kw = dict(signal="state_vartheta", scale=180 / math.pi)
    calls = {"eval_episodes": lambda: env.eval_episodes(steps, packed[0], **kw),
             "population_one_policy": lambda: env.eval_population(steps, packed, n, **kw),
             "population_one_policy_lane_gains": lambda: env.eval_population(steps, packed, n, pid_ss=gains, **kw)}
    ts = {k: [] for k in calls}
    outs = {}
    for r in range(runs + 1):                     # round 0: the warm-up
        for name, fn in calls.items():            # alternated call by call
            env.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            if r:
                ts[name].append(time.perf_counter() - t0)
    res = {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)} for k, v in ts.items()}
    base = res["eval_episodes"]["median_s"]
    res["population_over_eval_episodes"] = res["population_one_policy"]["median_s"] / base
    res["lane_gains_over_population"] = (res["population_one_policy_lane_gains"]["median_s"] /
                                         res["population_one_policy"]["median_s"])
    same = lambda a, b: bool(((a == b) | (a.isnan() & b.isnan())).all())
    res["same_rows_as_eval_episodes"] = {k: all(same(outs[k][m], outs["eval_episodes"][m]) for m in outs[k])
                                         for k in calls if k != "eval_episodes"}
    res["envs"] = n
    print("kernel", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_population.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    res = {"tk": TK, "sample_time": ST, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "policies": policies_leg(a.runs), "gains": gains_leg(a.runs), "kernel": kernel_leg(a.runs)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
