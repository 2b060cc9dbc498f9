"""The update phase of a PPO iteration, the parent's paths against ABI 13's, alternated in one process,
medians of `--rounds` after a warm-up of each, torch.cuda.synchronize around every timed call:
  compute_gae   the torch loop (gae_kernel=False) against one b747_ppo_gae launch, at 65,536 x 64, 4,096 x 64 and
                4 envs x 2,048 steps (SB3's default shape); and the kernel alone (device events) against 17 B x T N at
                the HBM peak;
  train()       fused_update=True with one pair of calls per minibatch (epoch_call=False) against one b747_ppo_epoch
                per epoch, at the bench shape (65,536 x 64, minibatches of 65,536) and at a host-bound one (64 envs x
                256 steps, minibatches of 64); both paths draw the same permutations and must end on the same bits.
The baseline is always the parent's path, never the code under test.
--variants tag=lib.so,...: the kernel-alone time of A/B builds of the library that differ in the GAE kernel's
geometry (-DB747_GAE_BLOCK / -DB747_GAE_UNROLL), each in a child process of its own (B747_LIB_PATH).
Run: python tools/exp_ppo_epoch.py [--out profiles/ppo_epoch.json] [--rounds 5] [--variants b256_u8=tools/ab/x.so,...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_epoch.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--variants", default="", help="tag=path,... A/B libraries for the kernel-alone sweep")
ap.add_argument("--kernel-only", action="store_true", help="the kernel-alone times of the loaded library as one JSON line")
a = ap.parse_args()

GAE_SHAPES = [(65536, 64), (4096, 64), (4, 2048)]       # (envs, steps)
HBM_PEAK = 8.0e12                                       # B/s (spec)
GAE_BYTES_PER_ROW = 17                                  # rew, val 4 + 4, done 1 read; adv, ret 4 + 4 written

sweep = {}
if a.variants and not a.kernel_only:                    # children first: one process with the GPU open at a time
    for spec in [("product", "")] + [tuple(s.split("=", 1)) for s in a.variants.split(",")]:
        env = dict(os.environ)
        if spec[1]:
            env["B747_LIB_PATH"] = os.path.abspath(spec[1])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--rounds", str(a.rounds)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"variant {spec[0]} failed ({r.returncode}):\n{r.stderr[-2000:]}")
        sweep[spec[0]] = json.loads(r.stdout.strip().splitlines()[-1])

import torch  # noqa: E402

import bench  # noqa: E402
from b747_rl_ctrl_amd import _lib  # noqa: E402
from b747_rl_ctrl_amd.ppo import PPO, PPOConfig  # noqa: E402

dev = torch.device("cuda")
p = lambda x: x.data_ptr()


def gae_kernel_alone(envs, T, inner=20):
    """us per b747_ppo_gae launch on synthetic buffers: device events around `inner` launches, medians over rounds"""
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(7)
    rew, val = torch.randn(T, envs, device=dev, generator=g), torch.randn(T, envs, device=dev, generator=g)
    done = torch.rand(T, envs, device=dev, generator=g) < 0.02
    last = torch.randn(envs, device=dev, generator=g)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    stream = torch.cuda.current_stream().cuda_stream
    ts = []
    for rnd in range(a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            _lib.check(L.b747_ppo_gae(p(rew), p(val), p(done), p(last), T, envs, 0.99, 0.95, p(adv), p(ret), stream),
                       "b747_ppo_gae")
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            ts.append(1e3 * e0.elapsed_time(e1) / inner)
    return ts


def kernel_alone_table():
    out = {}
    for envs, T in GAE_SHAPES:
        ts = gae_kernel_alone(envs, T)
        out[f"{envs}x{T}"] = {"us_median": round(statistics.median(ts), 2), "us_spread": round(max(ts) - min(ts), 2)}
    return out


if a.kernel_only:
    print(json.dumps(kernel_alone_table()))
    sys.exit(0)


# ----------------------------------------------------------------------------------------------- compute_gae --
def gae_paths(envs, T):
    env = bench.make_env(envs, 0, True, dev, seed=98, sample_time=0.05)
    cfg = PPOConfig(n_steps=T, batch_size=65536)
    paths = {"torch_loop": PPO(env, cfg, seed=0, rollout_kernel=False, gae_kernel=False),
             "kernel": PPO(env, cfg, seed=0, rollout_kernel=False, gae_kernel=True)}
    g = torch.Generator(device=dev).manual_seed(7)
    first = paths["torch_loop"]
    first.rew_buf.copy_(torch.randn(T, envs, device=dev, generator=g))
    first.val_buf.copy_(torch.randn(T, envs, device=dev, generator=g))
    first.done_buf.copy_(torch.rand(T, envs, device=dev, generator=g) < 0.02)
    first.last_obs.copy_(env.obs)
    for name in ("rew_buf", "val_buf", "done_buf", "last_obs"):
        getattr(paths["kernel"], name).copy_(getattr(first, name))
    return paths


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


gae = {}
for envs, T in GAE_SHAPES:
    paths = gae_paths(envs, T)
    inner = {"torch_loop": 1, "kernel": 10}
    ts = {k: [] for k in paths}
    for rnd in range(a.rounds + 1):            # round 0: the warm-up, not counted
        for name, ppo in paths.items():
            dt = timed(lambda: ppo.compute_gae(T), inner[name])
            if rnd:
                ts[name].append(dt)
    same = bool(torch.equal(paths["kernel"].adv_buf, paths["torch_loop"].adv_buf)
                and torch.equal(paths["kernel"].ret_buf, paths["torch_loop"].ret_buf))
    med = {k: statistics.median(v) for k, v in ts.items()}
    gae[f"{envs}x{T}"] = {
        "envs": envs, "steps": T, "calls_per_timed_window": inner,
        "compute_gae_us": {k: {"median": round(1e6 * med[k], 1), "spread": round(1e6 * (max(v) - min(v)), 1),
                               "all": [round(1e6 * x, 1) for x in v]} for k, v in ts.items()},
        "ratio_torch_loop_over_kernel": round(med["torch_loop"] / med["kernel"], 1),
        "adv_and_ret_bit_identical": same,
    }
    del paths
    torch.cuda.empty_cache()

alone = kernel_alone_table()
big = alone["65536x64"]
bytes_big = GAE_BYTES_PER_ROW * 65536 * 64
alone["65536x64"].update({"bytes": bytes_big, "us_at_hbm_peak_8TBs": round(1e6 * bytes_big / HBM_PEAK, 2),
                          "share_of_hbm_peak": round(1e6 * bytes_big / HBM_PEAK / big["us_median"], 3),
                          "note": "71 MB of buffers, launched back to back: they fit the 256 MiB Infinity Cache, so "
                                  "this is not a cold-HBM time"})


# --------------------------------------------------------------------------------------------------- train() --
def train_paths(envs, T, batch):
    paths = {}
    for name in ("per_minibatch_calls", "epoch_call"):
        env = bench.make_env(envs, 0, True, dev, seed=98, sample_time=0.05)
        ppo = PPO(env, PPOConfig(n_steps=T, batch_size=batch), seed=0, fused_update=True,
                  epoch_call=(name == "epoch_call"))
        ppo.last_obs.copy_(env.obs)
        ppo.collect_rollouts(T)
        ppo.compute_gae(T)
        paths[name] = ppo
    a_, b_ = paths.values()
    for name in ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf"):
        getattr(b_, name).copy_(getattr(a_, name))                          # the same rollout in both
    return paths


train = {}
for label, (envs, T, batch) in {"bench_shape": (65536, 64, 65536), "host_bound_shape": (64, 256, 64)}.items():
    paths = train_paths(envs, T, batch)
    gen = torch.Generator(device=dev)
    ts = {k: [] for k in paths}
    for rnd in range(a.rounds + 1):
        for name, ppo in paths.items():
            gen.manual_seed(1000 + rnd)        # the same permutations for both paths in a round
            order = lambda epoch, T_, n: torch.randperm(T_ * n, device=dev, generator=gen)
            dt = timed(lambda: ppo.train(T, minibatch_order=order), 1)
            if rnd:
                ts[name].append(dt)
    x, y = paths["per_minibatch_calls"], paths["epoch_call"]
    same = bool(torch.equal(x.flat[:x.n_params], y.flat[:y.n_params]) and torch.equal(x.upd_m, y.upd_m)
                and torch.equal(x.upd_v, y.upd_v) and torch.equal(x.upd_t, y.upd_t))
    med = {k: statistics.median(v) for k, v in ts.items()}
    spread = {k: max(v) - min(v) for k, v in ts.items()}
    n_mb = x.cfg.n_epochs * -(-envs * T // batch)
    train[label] = {
        "envs": envs, "steps": T, "batch_size": batch, "epochs": x.cfg.n_epochs, "minibatch_steps": n_mb,
        "train_seconds": {k: [round(v_, 5) for v_ in v] for k, v in ts.items()},
        "median_seconds": {k: round(v, 5) for k, v in med.items()},
        "spread_seconds": {k: round(v, 5) for k, v in spread.items()},
        "us_per_minibatch": {k: round(1e6 * v / n_mb, 2) for k, v in med.items()},
        "ratio_per_minibatch_calls_over_epoch_call": round(med["per_minibatch_calls"] / med["epoch_call"], 3),
        "epoch_call_no_slower_beyond_the_spread": bool(med["epoch_call"] - med["per_minibatch_calls"]
                                                       <= spread["epoch_call"] + spread["per_minibatch_calls"]),
        "parameters_and_moments_bit_identical": same,
    }
    del paths
    torch.cuda.empty_cache()

out = {
    "what": "compute_gae and PPO.train(fused_update=True): the parent's paths (torch loop; two calls per minibatch) "
            "against b747_ppo_gae and b747_ppo_epoch, alternated in one process, medians over the rounds after a warm-up",
    "rounds": a.rounds,
    "compute_gae": gae, "gae_kernel_alone": alone, "gae_geometry_sweep_kernel_alone_us": sweep or None, "train": train,
    "device": torch.cuda.get_device_name(0),
}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
