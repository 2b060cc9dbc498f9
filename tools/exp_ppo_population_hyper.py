"""Wall time of one PopulationPPO compute_gae + train with per-member hyper-parameters from the device table
(PopulationPPO(hyper=...): b747_ppo_gae_population, b747_ppo_epoch_batched_hyper) against the
shared-scalar path the library had before it (hyper=None: b747_ppo_gae, b747_ppo_epoch_batched), in one process on one
GPU.  P = 64 members of 64 envs, T = 64 (4,096 rows per member), batch_size 1,024 (4 minibatches of 16 workgroups per
member and epoch), n_epochs 10, batched_update=True; every row of the table holds cfg's values, so both paths do the
same arithmetic -- asserted bit for bit after the warm-up round and after the last.  The sample orders are drawn once
and reused (the same for both paths), so the timed region is the GAE launch, the epoch calls, the repack and train()'s
statistics.  The two populations alternate round by round; medians of --runs after a warm-up round,
torch.cuda.synchronize around every timed part; spread = max - min.
  python tools/exp_ppo_population_hyper.py [--out profiles/ppo_population_hyper.json] [--runs 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

P, EPP, T, BATCH, EPOCHS, ST, TK = 64, 64, 64, 1024, 10, 0.05, 20.0
SEED = 1


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "spread_s": max(ts) - min(ts)}


def population(hyper):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    env = BatchControllerEnv(P * EPP, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=TK, sample_time=ST, seed=3)
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS)
    return PopulationPPO(env, P, EPP, cfg, seed=SEED, batched_update=True, hyper=[{}] * P if hyper else None,
                         learning_rates=[3e-4 * (1 + (p % 5) * 0.5) for p in range(P)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_population_hyper.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    pops = {"shared_scalars": population(False), "hyper_table": population(True)}
    g = torch.Generator().manual_seed(7)
    orders = torch.stack([torch.stack([torch.randperm(T * EPP, generator=g) for _ in range(P)])
                          for _ in range(EPOCHS)]).cuda()
    order = lambda epoch, T_, n, p: orders[epoch, p]
    for pp in pops.values():
        pp.env.reset()
        pp.collect_rollouts(T)
    torch.cuda.synchronize()

    def same_bits():
        x, y = pops.values()
        torch.cuda.synchronize()
        return all(torch.equal(getattr(x, k), getattr(y, k)) for k in ("rew_buf", "adv_buf", "ret_buf", "flat", "upd_m",
                                                                       "upd_v", "upd_t"))
    ts = {name: {"gae": [], "train": [], "gae_and_train": []} for name in pops}
    for r in range(a.runs + 1):                 # round 0: the warm-up
        for name, pp in pops.items():           # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pp.compute_gae(T)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            pp.train(T, order)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r:
                ts[name]["gae"].append(t1 - t0)
                ts[name]["train"].append(t2 - t1)
                ts[name]["gae_and_train"].append(t2 - t0)
        assert same_bits(), f"the two paths differ after round {r}"
    res = {"what": __doc__.split("\n  python")[0], "members": P, "envs_per_member": EPP, "T": T, "batch_size": BATCH,
           "n_epochs": EPOCHS, "runs": a.runs, "device": torch.cuda.get_device_name(0), "same_bits": True}
    for name in pops:
        res[name] = {part: summary(v) for part, v in ts[name].items()}
    x, y = res["shared_scalars"]["gae_and_train"], res["hyper_table"]["gae_and_train"]
    res["hyper_over_shared"] = y["median_s"] / x["median_s"]
    res["difference_s"] = y["median_s"] - x["median_s"]
    res["beyond_both_spreads"] = abs(res["difference_s"]) > x["spread_s"] + y["spread_s"]
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
