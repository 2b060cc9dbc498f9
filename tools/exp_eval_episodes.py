"""Wall time and peak device memory of the two evaluation paths in one process:
  loop   evaluate.run_step_tests -- one recording launch per env step, driven by the packed policy through
         b747_policy_act (zero noise), the [steps, n_sub, N] history reduced at the end;
  fused  evaluate.run_step_tests_fused -- every episode in one b747_eval_episodes launch.
Sizes: (a) the callback's 4 envs, (b) 4,096 envs, both tk 20 s / sample_time 0.05 (400 env steps, 2,000 DLL steps);
the fused path alone at 65,536 envs.  Median of 5 runs after a warm-up, torch.cuda.synchronize around each.
  python tools/exp_eval_episodes.py [--out profiles/eval_episodes.json] [--runs 5]"""
import argparse
import ctypes
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


def two_launch_policy(net, obs_dim):
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.evaluate import packed_policy
    L = _lib.lib()
    flat = packed_policy(net, obs_dim, torch.device("cuda", torch.cuda.current_device()))
    bufs = {}

    def act(obs):
        n = obs.shape[0]
        if n not in bufs:
            bufs[n] = [torch.zeros(n, dtype=torch.float32, device=obs.device) for _ in range(5)]
        noise, a, logp, val, env_a = bufs[n]
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(L.b747_policy_act(p(flat), obs_dim, n, p(obs), p(noise), 0, None, 0, 0, None, p(a), p(logp), p(val),
                                     p(env_a), -1.0, 1.0, torch.cuda.current_stream().cuda_stream), "b747_policy_act")
        return env_a
    return act


def measure(fn, runs):
    fn()                                          # warm-up (module loads, allocator)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        del out
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
            "peak_bytes": int(torch.cuda.max_memory_allocated() - base)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_episodes.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    from b747_rl_ctrl_amd.evaluate import run_step_tests, run_step_tests_fused
    from b747_rl_ctrl_amd.ppo import ActorCritic
    torch.manual_seed(0)
    net = ActorCritic(3).cuda()
    act = two_launch_policy(net, 3)
    kw = dict(tk=TK, sample_time=ST)
    res = {"tk": TK, "sample_time": ST, "runs": a.runs, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (4, 4096, 65536):
        rep = n // len(REFS)
        row = {"fused": measure(lambda: run_step_tests_fused(net, REFS, replicas=rep, **kw), a.runs)}
        if n <= 4096:
            row["loop"] = measure(lambda: run_step_tests(act, REFS, replicas=rep, **kw), a.runs)
            row["speedup"] = row["loop"]["median_s"] / row["fused"]["median_s"]
        res["sizes"][str(n)] = row
        print(n, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
