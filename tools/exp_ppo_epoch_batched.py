"""Wall time of the member-batched PPO update (b747_ppo_epoch_batched) against the path the library had
before it (b747_ppo_epoch_population: a host loop over the members), in one process on one GPU:
  epoch      one epoch call for P = 1, 16 and 256 members of 64 envs on one real rollout (T = 64: 4,096 rows per
             member), at batch_size 4,096 (one minibatch of 64 workgroups per member) and 256 (16 minibatches of 4
             workgroups).  The two paths alternate call by call on two copies of the same state, which therefore stay
             equal: asserted bit for bit after the warm-up round and again after the last.  Every baseline call runs
             all P members: nothing is extrapolated.
  iteration  one PopulationPPO iteration at P = 16 and 256, n_epochs 10, one minibatch per member and epoch, split into
             collect / GAE / train (the epochs) / repack, each between torch.cuda.synchronize calls, for
             batched_update False and True.
  --profile B no timing: two epoch calls of each path at P = 16 and batch_size B, to be run under a kernel trace
             (per-kernel times; no counters in that run).
PID_LIKE / DIRECT_CONTROL / CONST, sample_time 0.05.  Medians of --runs after a warm-up, torch.cuda.synchronize around
every timed call; spread = max - min.
  python tools/exp_ppo_epoch_batched.py [--out profiles/ppo_epoch_batched.json] [--runs 5] [--profile 4096]"""
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
SEED = 1


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "spread_s": max(ts) - min(ts)}


def make_env(n):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=TK, sample_time=ST, seed=3)


def population(P, batch, n_epochs, batched):
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    cfg = PPOConfig(n_steps=T, batch_size=batch, n_epochs=n_epochs)
    return PopulationPPO(make_env(P * EPP), P, EPP, cfg, seed=SEED, batched_update=batched,
                         learning_rates=[3e-4 * (1 + (p % 5) * 0.5) for p in range(P)],
                         rew_configs=[{"k0": 1.0 + (p % 7) * 0.25} for p in range(P)])


class EpochCalls:
    """One rollout of a PopulationPPO and two copies of its update state: `baseline` and `batched` run one epoch each"""

    def __init__(self, P, batch):
        from b747_rl_ctrl_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.pp = pp = population(P, batch, 1, True)
        pp.env.reset()
        pp.collect_rollouts(T)
        pp.compute_gae(T)
        self.P, self.batch, self.n_rows = P, batch, T * EPP
        self.n_mb = -(-self.n_rows // batch)
        g = torch.Generator().manual_seed(7)
        local = torch.stack([torch.randperm(self.n_rows, generator=g) for _ in range(P)]).to(pp.env.device)
        self.perm = torch.gather(pp.member_rows(T), 1, local).contiguous()
        z = lambda: {"theta": pp.flat.clone(), "m": torch.zeros_like(pp.upd_m), "v": torch.zeros_like(pp.upd_v),
                     "t": torch.zeros_like(pp.upd_t),
                     "stats": torch.zeros(P, self.n_mb, 8, dtype=torch.float32, device=pp.env.device)}
        self.a, self.b = z(), z()
        torch.cuda.synchronize()

    def _head(self, s):
        pp, p = self.pp, lambda x: x.data_ptr()
        c = pp.cfg
        return (p(s["theta"]), self.P, pp.stride, pp.env.obs_dim, p(pp.obs_buf), p(pp.act_buf), p(pp.logp_buf),
                p(pp.adv_buf), p(pp.ret_buf), p(self.perm), self.n_rows, self.batch, c.clip_range, c.ent_coef, c.vf_coef)

    def baseline(self):
        pp, s, p = self.pp, self.a, lambda x: x.data_ptr()
        self._lib.check(self.L.b747_ppo_epoch_population(
            *self._head(s), p(pp.upd_ws), p(pp.upd_grad), p(s["m"]), p(s["v"]), p(s["t"]), pp.cfg.max_grad_norm, pp._lr,
            0.9, 0.999, 1e-5, p(s["stats"]), torch.cuda.current_stream().cuda_stream), "b747_ppo_epoch_population")

    def batched(self):
        pp, s, p = self.pp, self.b, lambda x: x.data_ptr()
        self._lib.check(self.L.b747_ppo_epoch_batched(
            *self._head(s), p(pp.upd_ws_batched), pp.upd_ws_batched.numel(), p(s["m"]), p(s["v"]), p(s["t"]),
            pp.cfg.max_grad_norm, p(pp.lr_dev), 0.9, 0.999, 1e-5, p(s["stats"]),
            torch.cuda.current_stream().cuda_stream), "b747_ppo_epoch_batched")

    def same_bits(self):
        torch.cuda.synchronize()
        return all(torch.equal(self.a[k], self.b[k]) for k in self.a) and bool(torch.isfinite(self.a["stats"]).all())


def epoch_leg(runs):
    out = {}
    for batch in (T * EPP, 256):
        for P in (1, 16, 256):
            ec = EpochCalls(P, batch)
            calls = {"population": ec.baseline, "batched": ec.batched}
            ts = {name: [] for name in calls}
            for r in range(runs + 1):             # round 0: the warm-up
                for name, fn in calls.items():    # alternated call by call
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r:
                        ts[name].append(time.perf_counter() - t0)
                if r == 0:
                    assert ec.same_bits(), "the two paths differ after one epoch"
            assert ec.same_bits(), "the two paths differ after the timed epochs"
            row = {name: summary(v) for name, v in ts.items()}
            row.update(members=P, batch_size=batch, minibatches=ec.n_mb, same_bits=True, extrapolated=False,
                       workspace_members=ec.pp.upd_ws_batched.numel() //
                       int(ec.L.b747_ppo_epoch_batched_workspace(ec.pp.env.obs_dim, batch)),
                       launches={"population": 4 * P * ec.n_mb, "batched": 4 * ec.n_mb})
            row["speedup"] = row["population"]["median_s"] / row["batched"]["median_s"]
            row["beyond_both_spreads"] = (row["population"]["median_s"] - row["batched"]["median_s"] >
                                          row["population"]["spread_s"] + row["batched"]["spread_s"])
            out[f"batch_{batch}_members_{P}"] = row
            print("epoch", batch, P, json.dumps(row), flush=True)
            del ec
    return out


def iteration_leg(runs):
    out = {}
    for P in (16, 256):
        for batched in (False, True):
            pp = population(P, T * EPP, 10, batched)
            pp.env.reset()
            parts = {"collect": lambda: pp.collect_rollouts(T), "gae": lambda: pp.compute_gae(T),
                     "train": lambda: pp.train(T), "repack": pp.repack}
            ts = {name: [] for name in parts}
            for r in range(runs + 1):             # round 0: the warm-up
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
            row["launches_per_train"] = 4 * (1 if batched else P) * pp.cfg.n_epochs + 1
            out[f"members_{P}_{'batched' if batched else 'population'}"] = row
            print("iteration", P, batched, json.dumps(row), flush=True)
            del pp
    return out


def profile_leg(batch):
    ec = EpochCalls(16, batch)
    for _ in range(2):
        ec.baseline()
        ec.batched()
    assert ec.same_bits()
    print("profile", batch, "ok", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_epoch_batched.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--profile", type=int, default=0, metavar="BATCH_SIZE")
    a = ap.parse_args()
    if a.profile:
        profile_leg(a.profile)
        return
    res = {"T": T, "envs_per_member": EPP, "sample_time": ST, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "epoch": epoch_leg(a.runs), "iteration": iteration_leg(a.runs)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
