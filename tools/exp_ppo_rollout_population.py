"""Wall time of the population PPO rollout (b747_ppo_rollout_population) against the path the library had
before it, in one process on one GPU:
  rollout     P members x 64 envs in ONE population call (a policy and a reward row per member) against P sequential
              b747_ppo_rollout_lanes calls on P 64-env batches (envs and buffers built beforehand; only the calls are
              timed).  Above 16 members 16 sequential calls are timed and the figure is scaled to P: "extrapolated".
  one_member  P = 1, no reward rows, against b747_ppo_rollout_lanes on the same batch, alternated call by call, at 64
              and 65,536 envs for obs_dim 3 (where that call defers the value head to a batched pass) and 5.
  learn       one PopulationPPO iteration at P = 16 and 256, n_epochs 10, one minibatch per member and epoch, split
              into collect / GAE / train (the epochs) / repack, each between torch.cuda.synchronize calls.
PID_LIKE (SPEED_MODE for obs_dim 5) / DIRECT_CONTROL / CONST, sample_time 0.05, T = 64.  Medians of --runs after a
warm-up, torch.cuda.synchronize around every timed call; spread = max - min.
  python tools/exp_ppo_rollout_population.py [--out profiles/ppo_rollout_population.json] [--runs 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, EPP, ST, TK = 64, 64, 0.05, 20.0
SEQ_MAX = 16
SEED = 1


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "spread_s": max(ts) - min(ts)}


def measure(fn, runs):
    fn()                                          # warm-up (module loads, allocator)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return summary(ts)


def scaled(m, factor, count):
    out = {k: v * factor for k, v in m.items()}
    out["calls_timed"] = count
    out["extrapolated"] = factor != 1.0
    return out


def make_env(n, obs="PID_LIKE", offset=0):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    return BatchControllerEnv(n, ObservationType[obs], RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=TK, sample_time=ST, seed=3,
                              env_offset=offset)


class Buffers:
    def __init__(self, env):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=env.device)
        n, od = env.n, env.obs_dim
        self.env = env
        self.bufs = (z(T, n, od), z(T, n, 1), z(T, n), z(T, n), z(T, n), z(T, n, dt=torch.bool))
        self.step_base = torch.zeros(1, dtype=torch.int64, device=env.device)
        self.last_val = z(n)

    def lanes(self, flat):
        from b747_rl_ctrl_amd import _lib
        env, p = self.env, lambda x: x.data_ptr()
        env._batch().action = p(env.action)
        _lib.check(_lib.lib().b747_ppo_rollout_lanes(env._bref, env._cref, env._kref, p(flat), SEED, p(self.step_base), T,
                                                     *(p(b) for b in self.bufs), -1.0, 1.0,
                                                     torch.cuda.current_stream().cuda_stream), "b747_ppo_rollout_lanes")

    def population(self, flat, epp, rew_pop):
        self.env.ppo_rollout_population(T, flat, *self.bufs, seed=SEED, step_base=self.step_base, envs_per_policy=epp,
                                        rew_pop=rew_pop, last_val=self.last_val)


def nets_of(od, count):
    from b747_rl_ctrl_amd.ppo import ActorCritic
    torch.manual_seed(0)
    return [ActorCritic(od) for _ in range(count)]


def rollout_leg(runs):
    from b747_rl_ctrl_amd.evaluate import pack_policies, packed_policy
    nets = nets_of(3, SEQ_MAX)
    base = torch.stack([n.flat_params().detach() for n in nets])
    seq = [Buffers(make_env(EPP, offset=p * EPP)) for p in range(SEQ_MAX)]
    seq_flat = [packed_policy(n, 3, seq[0].env.device) for n in nets]
    out = {}
    for P in (1, 16, 256, 1024):
        pop = Buffers(make_env(P * EPP))
        flat = pack_policies(base[torch.arange(P) % SEQ_MAX] + 1e-3 * torch.randn(P, base.shape[1]), 3, pop.env.device)
        rew = torch.tensor([pop.env.rew_constants({"k0": 1.0 + (p % 7) * 0.25, "kf": 0.05 + (p % 5) * 0.05,
                                                   "k1": 1 + p % 4}) for p in range(P)],
                           dtype=torch.float64, device=pop.env.device)
        k = min(P, SEQ_MAX)

        def sequential():
            for p in range(k):
                seq[p].lanes(seq_flat[p])
        row = {"envs": P * EPP, "population": measure(lambda: pop.population(flat, EPP, rew), runs),
               "sequential": scaled(measure(sequential, runs), P / k, k)}
        row["speedup"] = row["sequential"]["median_s"] / row["population"]["median_s"]
        row["beyond_both_spreads"] = (row["sequential"]["median_s"] - row["population"]["median_s"] >
                                      row["population"]["spread_s"] + row["sequential"]["spread_s"])
        out[str(P)] = row
        print("rollout", P, json.dumps(row), flush=True)
        del pop
    return out


def one_member_leg(runs):
    from b747_rl_ctrl_amd.evaluate import packed_policy
    out = {}
    for obs, od in (("PID_LIKE", 3), ("SPEED_MODE", 5)):
        net = nets_of(od, 1)[0]
        for n in (64, 65536):
            run = Buffers(make_env(n, obs))
            flat = packed_policy(net, od, run.env.device)
            calls = {"rollout_lanes": lambda: run.lanes(flat),
                     "population_one_member": lambda: run.population(flat.view(1, -1), n, None)}
            ts = {name: [] for name in calls}
            for r in range(runs + 1):             # round 0: the warm-up
                for name, fn in calls.items():    # alternated call by call
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r:
                        ts[name].append(time.perf_counter() - t0)
            row = {name: summary(v) for name, v in ts.items()}
            row["population_over_lanes"] = row["population_one_member"]["median_s"] / row["rollout_lanes"]["median_s"]
            out[f"obs_dim_{od}_envs_{n}"] = row
            print("one_member", od, n, json.dumps(row), flush=True)
            del run
    return out


def learn_leg(runs):
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    out = {}
    for P in (16, 256):
        cfg = PPOConfig(n_steps=T, batch_size=T * EPP, n_epochs=10)
        pp = PopulationPPO(make_env(P * EPP), P, EPP, cfg, seed=SEED,
                           rew_configs=[{"k0": 1.0 + (p % 7) * 0.25} for p in range(P)])
        pp.env.reset()
        parts = {"collect": lambda: pp.collect_rollouts(T), "gae": lambda: pp.compute_gae(T), "train": lambda: pp.train(T),
                 "repack": pp.repack}
        ts = {name: [] for name in parts}
        for r in range(runs + 1):                 # round 0: the warm-up
            for name, fn in parts.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r:
                    ts[name].append(time.perf_counter() - t0)
        row = {name: summary(v) for name, v in ts.items()}
        # train() ends with the repack and one host read of the statistics: the epochs are the rest
        row["epochs_median_s"] = row["train"]["median_s"] - row["repack"]["median_s"]
        total = row["collect"]["median_s"] + row["gae"]["median_s"] + row["train"]["median_s"]
        row["iteration_median_s"] = total
        row["share"] = {"collect": row["collect"]["median_s"] / total, "gae": row["gae"]["median_s"] / total,
                        "epochs": row["epochs_median_s"] / total, "repack": row["repack"]["median_s"] / total}
        row["launches_per_train"] = 4 * P * cfg.n_epochs + 1
        out[str(P)] = row
        print("learn", P, json.dumps(row), flush=True)
        del pp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_rollout_population.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    res = {"T": T, "envs_per_member": EPP, "sample_time": ST, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "rollout": rollout_leg(a.runs), "one_member": one_member_leg(a.runs), "learn": learn_leg(a.runs)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
