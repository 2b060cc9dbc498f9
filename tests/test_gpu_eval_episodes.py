"""Whole evaluation episodes in one launch (b747_eval_episodes: BatchControllerEnv.eval_episodes,
evaluate.run_step_tests_fused / monte_carlo_step_tests) against the paths the project already has:

  1. run_step_tests (one recording launch per env step + the torch reduction over the history) driven by the same
     packed policy through b747_policy_act with zero noise (action = clip(mean)), FAST and FAITHFUL, PID_LIKE /
     SPEED_MODE, DIRECT / ADD_DIRECT control;
  2. with no policy (the PID baseline: AUTO, sample_time = dt), the CPU restatement of the reference
     (oracle/ref_env.py + calc_stepinfo) -- independent of every GPU path;
  3. a partial wave (70 envs): the same results as the 4-env launch;
  4. episodes that end early (the limiter): length, ITSE and the metrics as run_step_tests cuts them, the env left at
     its first done;
  5. the reference DLL's own recorded ControlTestCallback metrics (tests/golden/tb_transfer_first_log.json);
  6. Monte-Carlo episodes: identical however the batch is sharded.

Tolerances of 1-4 are those of tests/test_gpu_evaluate.py (the closed loop a = -3 obs[1] it shows to be well
conditioned): overshoot 1e-3 relative, rise / settling time within one DLL sample (0.0100001 s), static error 1e-5
deg, quality 1e-6 relative; lengths equal.  Shapes: 4 envs (the callback's references), tk 10 s, sample_time 0.05:
200 env steps, 1,000 DLL steps."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from stepinfo_ref import calc_stepinfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_env as R  # noqa: E402
import tb_transfer as T  # noqa: E402

pytestmark = pytest.mark.gpu

REFS = [5 * math.pi / 180, -5 * math.pi / 180, 10 * math.pi / 180, -10 * math.pi / 180]   # neural/agent.py:117
STATE0 = [0, 11000, 250, 0, 0, 0]
TK, ST = 10.0, 0.05
METRICS = ("overshoot", "rise_time", "settling_time", "static_error", "quality")


def _linear_policy(obs_dim):
    """An ActorCritic whose policy head is the near-linear law a = -60 tanh(tanh(0.05 obs[1])) ~ -3 obs[1]"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    net = ActorCritic(obs_dim)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        net.pi_net[0].weight[0, 1] = 0.05
        net.pi_net[2].weight[0, 0] = 1.0
        net.action_net.weight[0, 0] = -60.0
    return net


def _weights_policy(weights, obs_dim):
    """An ActorCritic with the given policy-head weights [(W, b)] x 3 (tests/tb_transfer.py reference_weights)"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    net = ActorCritic(obs_dim)
    with torch.no_grad():
        for lin, (w, b) in zip((net.pi_net[0], net.pi_net[2], net.action_net), weights):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    return net


def _two_launch_policy(net, obs_dim, lo=-1.0, hi=1.0):
    """obs -> clip(mean) through b747_policy_act with zero noise: the policy arithmetic of the rollout kernels (f16
    hi/lo matrix-core products), one launch per call -- what run_step_tests is driven with"""
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
        assert obs.dtype == torch.float32 and obs.is_contiguous()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(L.b747_policy_act(p(flat), obs_dim, n, p(obs), p(noise), 0, None, 0, 0, None, p(a), p(logp), p(val),
                                     p(env_a), lo, hi, torch.cuda.current_stream().cuda_stream), "b747_policy_act")
        return env_a
    return act, flat


def _same(a, b):
    """torch.equal with NaN == NaN (rise / settling time are NaN where calc_stepinfo gives None)"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _close(fused, loop, j, ctx):
    f = lambda o, k: float(o[k][j])
    assert f(fused, "overshoot") == pytest.approx(f(loop, "overshoot"), rel=1e-3), ctx
    for k in ("rise_time", "settling_time"):
        if math.isnan(f(loop, k)):
            assert math.isnan(f(fused, k)), (ctx, k)
        else:
            assert abs(f(fused, k) - f(loop, k)) <= 0.0100001, (ctx, k, f(fused, k), f(loop, k))
    assert f(fused, "static_error") == pytest.approx(f(loop, "static_error"), abs=1e-5), ctx
    assert f(fused, "quality") == pytest.approx(f(loop, "quality"), rel=1e-6), ctx


def _kw(obs="PID_LIKE", mode="DIRECT_CONTROL", variant="fast", tk=TK):
    from b747_rl_ctrl_amd import CtrlMode, ObservationType
    m, amax = T.MODES[mode]
    return dict(state0=STATE0, tk=tk, observation_type=ObservationType(T.OBS[obs]), ctrl_mode=CtrlMode(m),
                sample_time=ST, action_max=amax, variant=variant)


@pytest.fixture(scope="module")
def fused4():
    """the 4-env FAST PID_LIKE / DIRECT run of the fused path, shared by the tests that compare against it"""
    from b747_rl_ctrl_amd.evaluate import run_step_tests_fused
    out = run_step_tests_fused(_linear_policy(3), REFS, **_kw())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("obs,mode,variant", [("PID_LIKE", "DIRECT_CONTROL", "fast"),
                                              ("PID_LIKE", "DIRECT_CONTROL", "faithful"),
                                              ("SPEED_MODE", "DIRECT_CONTROL", "fast"),
                                              ("PID_LIKE", "ADD_DIRECT_CONTROL", "fast")])
def test_fused_episodes_match_the_step_loop(obs, mode, variant, fused4):
    from b747_rl_ctrl_amd.evaluate import run_step_tests, run_step_tests_fused
    od = T.OBS_DIM[obs]
    net = _linear_policy(od)
    act, _ = _two_launch_policy(net, od)
    loop = run_step_tests(act, REFS, **_kw(obs, mode, variant))
    fused = fused4 if (obs, mode, variant) == ("PID_LIKE", "DIRECT_CONTROL", "fast") else \
        run_step_tests_fused(net, REFS, **_kw(obs, mode, variant))
    assert bool(loop["done"].all()) and bool(fused["done"].all())
    assert torch.equal(fused["length"], loop["length"]) and int(fused["length"][0]) == 1000
    for j in range(len(REFS)):
        _close(fused, loop, j, (obs, mode, variant, j))
    assert float(fused["mean_quality"]) == pytest.approx(float(fused["quality"].mean()))


def test_ppo_step_tests_uses_the_packed_policy(fused4):
    """PPO.step_tests (the training-loop callback) = run_step_tests_fused with PPO.flat"""
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, RewardType
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    env = BatchControllerEnv(64, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, sample_time=ST, tk=TK)
    ppo = PPO(env, PPOConfig(n_steps=4))
    ppo.policy.load_state_dict(_linear_policy(3).state_dict())
    ppo.sync_params()
    out = ppo.step_tests(REFS, state0=STATE0)
    for k in METRICS + ("length",):
        assert _same(out[k], fused4[k]), k


def _cpu_pid_episode(vref):
    """_cpu_episode of tests/test_gpu_evaluate.py with the SS PID flying (AUTO, action ignored, sample_time = dt)"""
    c = R.RefController(1, None, None, None, tk=TK, sample_time=None)
    e = R.RefControllerEnv(0, 0, True, True, c)
    e.reset({"state0": np.array(STATE0, float), "kind": "const", "ref": vref, "aero_err": None})
    t, th = [], []

    def rec(m):
        t.append(m.time)
        th.append(float(np.nan_to_num(m.state[4])) * 180 / math.pi)
    done = False
    while not done:
        _, _, done = e.step(np.float32(0.0), rec)
    return calc_stepinfo(th, vref * 180 / math.pi, ts=t), c.quality(), len(th)


def test_pid_baseline_without_a_policy_matches_the_cpu_reference():
    from b747_rl_ctrl_amd import CtrlType
    from b747_rl_ctrl_amd.evaluate import run_step_tests_fused
    out = run_step_tests_fused(None, REFS, state0=STATE0, tk=TK, ctrl_type=CtrlType.AUTO, ctrl_mode=None,
                               sample_time=None)
    assert bool(out["done"].all())
    for j, vref in enumerate(REFS):
        info, q, n = _cpu_pid_episode(vref)
        assert int(out["length"][j]) == n == 1000
        assert float(out["overshoot"][j]) == pytest.approx(abs(info["overshoot"]), rel=1e-3)
        for k in ("rise_time", "settling_time"):
            if info[k] is None:
                assert math.isnan(float(out[k][j])), k
            else:
                assert abs(float(out[k][j]) - info[k]) <= 0.0100001, (k, float(out[k][j]), info[k])
        assert float(out["static_error"][j]) == pytest.approx(info["static_error"], abs=1e-5)
        assert float(out["quality"][j]) == pytest.approx(q, rel=1e-6)


def test_partial_wave_gives_the_same_episodes(fused4):
    from b747_rl_ctrl_amd.evaluate import run_step_tests_fused
    refs = (REFS * 18)[:70]                       # two waves, the second with 6 envs and 58 idle lanes
    out = run_step_tests_fused(_linear_policy(3), refs, **_kw())
    for k in METRICS + ("length", "return"):
        assert _same(out[k][:4], fused4[k]), k
        assert _same(out[k][64:70], out[k][0:6]), k
    assert _same(out["env"].X[:, 64:70], out["env"].X[:, 0:6]) and bool(out["done"].all())


def _constant(action):
    a = torch.as_tensor(action, dtype=torch.float32, device="cuda")
    return lambda obs: a.expand(obs.shape[0]).contiguous()


@pytest.mark.parametrize("action", [[-1.0] * 4, [-1.0, 0.0, -1.0, 0.0]], ids=["all_end_early", "two_run_to_tk"])
def test_episodes_that_end_early(action):
    from b747_rl_ctrl_amd.evaluate import run_step_tests, run_step_tests_fused
    kw = dict(_kw(), use_limiter=True)
    loop = run_step_tests(_constant(action), REFS, **kw)
    fused = run_step_tests_fused(None, REFS, action=action, **kw)
    full = int(round(TK / 0.01))
    early = torch.tensor([a != 0.0 for a in action], device="cuda")
    assert torch.equal(fused["length"], loop["length"])
    assert bool((fused["length"][early] < full).all()) and bool((fused["length"][~early] == full).all())
    assert bool(fused["done"].all())
    for j in range(4):
        _close(fused, loop, j, (action, j))
    env = fused["env"]                            # frozen at its first done
    assert torch.equal(env.k.to(torch.int64), fused["length"])
    assert torch.equal(env.ep_final_len.to(torch.int64) * int(env.cfg.n_sub), fused["length"])


def test_recorded_dll_runs_are_reproduced():
    """The reference DLL's recorded ControlTestCallback means (tk 20 s, 4 references) for the 7 distinct policies of
    the 17 reconstructible runs.  Settling time: the project's gate, 0.0025 + 1e-6 s.  Overshoot and quality: the
    error of the two-launch path (run_step_tests driven by b747_policy_act: the same f16 hi/lo policy arithmetic)
    against the record is measured first, and the fused path may be at most twice that from the record, and never
    held below 1e-6 -- the factor 2 covers summation-order and contraction differences between the HEADS = 1 policy
    head of the episode kernel and the two-head k_policy_act.  The gate comes from the two-launch path's error, not
    from the fused output.  Measured (MI355X, FAST; the test prints the table): the two-launch path against
    the record -- settling time equal in all 7, overshoot 0 to 1.1e-16, quality 0, 0, 2.05e-7, 0, 0, 6.49e-7, 1.28e-6 (in
    the order of the printed table) -- and the fused path's float32 means equal to the two-launch path's in all 21."""
    from b747_rl_ctrl_amd.evaluate import run_step_tests, run_step_tests_fused
    runs = T.load_fixture()
    seen = {}
    for name in sorted(runs):
        w = T.reference_weights(name)
        key = None if w is None else T.split_run(name) + (T.previous_obs(name),)
        if w is None or key in seen:
            continue
        obs, mode = T.split_run(name)
        od = T.OBS_DIM[obs]
        net = _weights_policy(w, od)
        kw = _kw(obs, mode, tk=T.TK)
        kw["state0"] = T.STATE0.tolist()
        act, _ = _two_launch_policy(net, od)
        means = lambda out: [float(out[k].double().mean().to(torch.float32)) for k in T.KEYS]
        two, fused = means(run_step_tests(act, T.REFS, **kw)), means(run_step_tests_fused(net, T.REFS, **kw))
        rec = runs[name]
        e2, ef = T.rel_err(two, rec), T.rel_err(fused, rec)
        seen[key] = (e2, ef)
        print(f"\n{name}: two-launch vs record settling {two[0] - rec['settling_time']:+.4f} s overshoot {e2[1]:.2e} "
              f"quality {e2[2]:.2e}; fused settling {fused[0] - rec['settling_time']:+.4f} s overshoot {ef[1]:.2e} "
              f"quality {ef[2]:.2e}")
        assert abs(fused[0] - rec["settling_time"]) <= 0.0025 + 1e-6, (name, fused, rec)
        for j in (1, 2):
            assert ef[j] <= max(2 * e2[j], 1e-6), (name, T.KEYS[j], fused[j], two[j], rec[T.KEYS[j]])
    assert len(seen) == 7


def test_monte_carlo_is_independent_of_the_sharding():
    from b747_rl_ctrl_amd.evaluate import monte_carlo_step_tests
    net = _linear_policy(3)
    whole = monte_carlo_step_tests(net, 256, seed=7, tk=5.0)
    parts = [monte_carlo_step_tests(net, 128, seed=7, tk=5.0, env_offset=off) for off in (0, 128)]
    for k in METRICS + ("length", "return", "vartheta_ref"):
        assert _same(whole[k], torch.cat([p[k] for p in parts])), k
    assert float(whole["overshoot_nan_share"]) == 0.0            # CONST references are never 0
    assert whole["overshoot_quantiles"].shape == (3,) and bool(whole["done"].all())
    assert bool((whole["vartheta_ref"].abs() >= math.pi / 180 - 1e-12).all())
    assert len(torch.unique(whole["vartheta_ref"])) > 200         # every env drew its own reference
