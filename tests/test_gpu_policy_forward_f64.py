"""Every inference form of the matrix-core policy forward (csrc/b747_policy.h) against ActorCritic(od).double() on the
CPU, at trained weight scales: policies scaled by g in {1, 3, 10}, observations from 1e-3 to 10 and mixed, with edge
rows at the f16 subnormal thresholds and around the +-65504 clamp.  The policies, observation sets, reference,
yardstick (the same module in fp32 on the CPU) and the bars are those of tests/test_policy_forward_model.py, whose
docstring states them:

    err(kernel) <= 16 err(torch32) + 2^-22 max(1, max |x64|)             (mean and value, per case)
    |logp - logp64(a)| <= (|z| / sigma) (B_mean + 2^-24 |a|) + 2^-22 max(1, |logp64|)            (per row)

Nothing is compared with another kernel's output.  The kernels are fed through _lib.lib():
  1. b747_policy_act (actor_critic<OD, 3>), od 3 / 5 / 7 / 8 / 10: noise = 0 makes act_out the mean to the bit; seeded
     noise at log_std 0 and -3 for the log-probability; b747_policy_pack_batch at a padded stride against
     b747_policy_pack.
  2. b747_ppo_rollout_lanes, T = 1, FAST and FAITHFUL: od 3 (actor_critic<3, 1> + the deferred k_policy_value<3>,
     two blocks, the second with 70 rows) and od 5 (<5, 1> and <5, 2> in the loop).  env.obs is overwritten with the
     observation set before the launch: the kernels take the first policy input from there.  log_std = -100: the f32
     standard deviation is below 1e-43, so act_buf[0] is the mean; a second launch at log_std = -3 gives logp_buf[0].
  3. b747_ppo_rollout (head_lds + the value pass), od 3, n = 1,088.
  4. b747_ppo_rollout_population, T = 1, n = 134 at 64 envs per policy: the members are g = 1, 3, 10 at a padded
     stride, each slice against its own float64 policy; last_val against the float64 value of env.obs after the launch.
  5. What the error does to training: a lanes rollout (T = 14, n = 70, g = 3, log_std = -3), then b747_ppo_grad over
     all its rows with old_logp = logp_buf.  The update's forward is fp64, so its ratio differs from 1 by the inference
     kernels' error alone: with delta the largest log-probability bound, clip fraction 0 and approx_kl <= delta^2 / 2
     (1 + delta).
Not covered: b747_eval_episodes and b747_eval_population show the mean only through the dynamics; they run
actor_critic<OD, 1>, as form 2 does.

Measured on one MI355X (DESIGN.md 16 has every case, with the CPU model's error on the same rows beside it):
err(kernel) / err(torch32) between 1.0 and 16.1 for the mean and 0.7 and 11.9 for the value over all forms and cases;
0.06 to 0.89 of the bar used (mean), 0.04 to 0.63 (value); the log-probability error 0.06 to 0.89 of its bound; the
kernels at 0.7 to 2.0 times the ideal model.  The largest share, 0.89, is b747_policy_act at od 5, g 3, randn x 1e-3
(the model is at 0.68 there: the design's error, against a yardstick taken on rows that are almost one point).  Form 5:
approx_kl 7.9e-11 (od 3) and 1.1e-9 (od 5) against bounds of 6.5e-8 and 1.8e-7, clip fraction 0.  One case needed a
margin, derived where it is applied: last_val of the od 3, g = 1 member."""
import pytest
import torch

from test_gpu_ppo_rollout_lanes import SENTINEL, _env as _lanes_env
from test_policy_forward_model import (GS, N_ROWS, SETS, bar, err, logp_check, model_forward, observations, policy,
                                       reference, yardstick)

pytestmark = pytest.mark.gpu

PAD = 8
NOISE_SEED, ROLLOUT_SEED = 5, 1
CONFIG = {3: ("PID_LIKE", "DIRECT_CONTROL", "CONST"), 5: ("SPEED_MODE", "ADD_DIRECT_CONTROL", "CONST")}
_p = lambda t: t.data_ptr()


def _dev():
    return torch.device("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _packed(net, od):
    from b747_rl_ctrl_amd.evaluate import packed_policy
    return packed_policy(net, od, _dev())


def _pack_wide(nets, od):
    """[P, num + PAD]: the policies packed in place by ONE b747_policy_pack_batch at the padded stride, the tail of
    every stride a sentinel"""
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    num = int(L.b747_policy_num_params(od))
    flat = torch.zeros(len(nets), num + PAD, device=_dev())
    flat[:, num:] = SENTINEL
    for q, net in enumerate(nets):
        fp = net.flat_params()
        flat[q, :fp.numel()].copy_(fp)
    _lib.check(L.b747_policy_pack_batch(_p(flat), od, len(nets), num + PAD, _stream()), "b747_policy_pack_batch")
    return flat, num


def _held(form, case, what, e, e32, b):
    """print the figures, then hold the kernel's error to the bar"""
    ratio = e / e32 if e32 > 0 else float("inf")
    print(f"F64 | {form} | {case} | {what} | err {e:.3e} | torch32 {e32:.3e} | ratio {ratio:.2f} | of bar {e / b:.3f}")
    assert e <= b, f"{form} {case} {what}: err {e:.3e} > bar {b:.3e} (torch32 {e32:.3e})"


def _mean_and_value_held(form, case, mean, value, ref):
    _held(form, case, "mean", err(mean.cpu(), ref["mean64"]), ref["err32_mean"], ref["bar_mean"])
    _held(form, case, "value", err(value.cpu(), ref["val64"]), ref["err32_val"], ref["bar_val"])


def _model_figures(form, case, net, obs, ref):
    """the CPU model's error on the same rows, beside the kernel's (printed only)"""
    mean, value = model_forward(net, obs.detach().cpu().float())
    print(f"F64 | {form} | {case} | model | mean {err(torch.from_numpy(mean), ref['mean64']):.3e} | "
          f"value {err(torch.from_numpy(value), ref['val64']):.3e}")


def _logp_held(form, case, logp, act, ref, log_std):
    diff, bound = logp_check(logp, act, ref["mean64"], log_std, ref["bar_mean"])
    worst = int((diff / bound).argmax())
    print(f"F64 | {form} | {case} | logp at log_std {log_std} | err {float(diff.max()):.3e} | "
          f"of bound {float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all()), \
        f"{form} {case} logp: row {worst}: {float(diff[worst]):.3e} > {float(bound[worst]):.3e}"
    return diff, bound


# ---------------------------------------------------------------- 1. b747_policy_act

def _act(flat, od, obs, noise):
    from b747_rl_ctrl_amd import _lib
    n = obs.shape[0]
    out = {k: torch.full((n,), SENTINEL, device=_dev()) for k in ("act", "logp", "val", "env")}
    out["obs"] = torch.full((n, od), SENTINEL, device=_dev())
    _lib.check(_lib.lib().b747_policy_act(_p(flat), od, n, _p(obs), _p(noise), 0, None, 0, 0, _p(out["obs"]),
                                          _p(out["act"]), _p(out["logp"]), _p(out["val"]), _p(out["env"]), -1.0, 1.0,
                                          _stream()), "b747_policy_act")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("od", [3, 5, 7, 8, 10])
def test_policy_act(od, g, name):
    ref, case = reference(od, g, name), f"od {od} g {g} {name}"
    obs = observations(od, name).to(_dev())
    out = _act(_packed(policy(od, g), od), od, obs, torch.zeros(N_ROWS, device=_dev()))
    assert torch.equal(out["obs"], obs), "obs_out"
    assert torch.equal(out["env"], out["act"].clamp(-1, 1)), "env_action"
    _mean_and_value_held("policy_act", case, out["act"], out["val"], ref)
    _model_figures("policy_act", case, policy(od, g), obs, ref)
    noise = torch.randn(N_ROWS, generator=torch.Generator().manual_seed(NOISE_SEED)).to(_dev())
    for log_std in (0.0, -3.0):
        out = _act(_packed(policy(od, g, log_std), od), od, obs, noise)
        assert torch.equal(out["obs"], obs) and torch.equal(out["env"], out["act"].clamp(-1, 1))
        _logp_held("policy_act", case, out["logp"], out["act"], ref, log_std)
        _held("policy_act", case, f"value at log_std {log_std}", err(out["val"].cpu(), ref["val64"]), ref["err32_val"],
              ref["bar_val"])


@pytest.mark.parametrize("od", [3, 5, 7, 8, 10])
def test_policy_pack_batch_at_a_padded_stride_is_policy_pack(od):
    nets = [policy(od, g) for g in GS]
    flat, num = _pack_wide(nets, od)
    torch.cuda.synchronize()
    assert bool((flat[:, num:] == SENTINEL).all()), "behind a policy's parameters within its stride"
    for q, net in enumerate(nets):
        single = _packed(net, od)
        assert single.numel() == num
        assert torch.equal(flat[q, :num].view(torch.int32), single.view(torch.int32)), f"policy {q} (g = {GS[q]})"


# ---------------------------------------------------------------- 2. - 5. the rollout kernels

class _Rollout:
    """an env whose observation is the given set, rollout buffers with a sentinel row T, and a Philox counter"""

    def __init__(self, env, T, obs=None):
        self.env, self.T = env, T
        n, od, dev = env.n, env.obs_dim, env.device
        env.track_episodes()
        if obs is not None:
            env.obs.copy_(obs.to(dev))
        full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)
        self.obs_buf, self.act_buf = full(T + 1, n, od), full(T + 1, n, 1)
        self.logp_buf, self.val_buf, self.rew_buf = full(T + 1, n), full(T + 1, n), full(T + 1, n)
        self.done_buf = torch.ones(T + 1, n, dtype=torch.bool, device=dev)
        self.step_base = torch.zeros(1, dtype=torch.int64, device=dev)
        self.last_val_all = full(n + PAD)
        self.last_val = self.last_val_all[:n]

    def single(self, entry, flat):
        """entry: b747_ppo_rollout_lanes or b747_ppo_rollout (the same arguments)"""
        from b747_rl_ctrl_amd import _lib
        env = self.env
        b = env._batch()
        b.action = _p(env.action)
        _lib.check(getattr(_lib.lib(), entry)(
            env._bref, env._cref, env._kref, _p(flat), ROLLOUT_SEED, _p(self.step_base), self.T, _p(self.obs_buf),
            _p(self.act_buf), _p(self.logp_buf), _p(self.val_buf), _p(self.rew_buf), _p(self.done_buf), -1.0, 1.0,
            _stream()), entry)
        return self._done()

    def population(self, flat, epp):
        self.env.ppo_rollout_population(self.T, flat, self.obs_buf, self.act_buf, self.logp_buf, self.val_buf,
                                        self.rew_buf, self.done_buf, seed=ROLLOUT_SEED, step_base=self.step_base,
                                        envs_per_policy=epp, rew_pop=None, last_val=self.last_val)
        return self._done()

    def _done(self):
        T = self.T
        torch.cuda.synchronize()
        assert int(self.step_base) == T
        for name in ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf"):
            assert bool((getattr(self, name)[T] == SENTINEL).all()), f"{name}: row T was written"
        assert bool(self.done_buf[T].all()), "done_buf: row T was written"
        assert bool((self.last_val_all[self.env.n:] == SENTINEL).all()), "past last_val[N]"
        return self


def _training_env(n):
    """the configuration b747_ppo_rollout covers (tests/test_gpu_ppo.py)"""
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, DisturbanceMode, ObservationType,
                                  ResetRefMode, RewardType)
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST,
                              disturbance_mode=DisturbanceMode.AERO_DISTURBANCE, tk=0.3, seed=3)


def _one_step(form, make_env, entry, od, g, name, n):
    """T = 1 of a single-policy rollout kernel on the observation set: mean, value, observation row, log-probability"""
    ref, case = reference(od, g, name, n), f"od {od} g {g} {name}"
    obs = observations(od, name, n)
    run = _Rollout(make_env(), 1, obs).single(entry, _packed(policy(od, g, -100.0), od))
    assert torch.equal(run.obs_buf[0].cpu().view(torch.int32), obs.view(torch.int32)), "obs_buf[0] is the set"
    _mean_and_value_held(form, case, run.act_buf[0], run.val_buf[0], ref)
    _model_figures(form, case, policy(od, g), obs, ref)
    run = _Rollout(make_env(), 1, obs).single(entry, _packed(policy(od, g, -3.0), od))
    _logp_held(form, case, run.logp_buf[0], run.act_buf[0], ref, -3.0)
    _held(form, case, "value at log_std -3", err(run.val_buf[0].cpu(), ref["val64"]), ref["err32_val"], ref["bar_val"])


@pytest.mark.parametrize("name", ["mixed", "s1e-3"])
@pytest.mark.parametrize("g", [1, 10])
@pytest.mark.parametrize("variant", ["fast", "faithful"])
@pytest.mark.parametrize("od", [3, 5])
def test_rollout_lanes_first_step(od, variant, g, name):
    o, m, r = CONFIG[od]
    _one_step(f"rollout_lanes {variant}", lambda: _lanes_env(o, m, r, variant, n=N_ROWS), "b747_ppo_rollout_lanes",
              od, g, name, N_ROWS)


@pytest.mark.parametrize("g", [1, 10])
def test_rollout_split_first_step(g):
    _one_step("rollout_split", lambda: _training_env(1088), "b747_ppo_rollout", 3, g, "mixed", 1088)


@pytest.mark.parametrize("od", [3, 5])
def test_rollout_population_first_step_members_at_their_own_scales(od):
    n, epp = 134, 64
    o, m, r = CONFIG[od]
    obs = observations(od, "mixed", n)
    slices = [slice(s, min(s + epp, n)) for s in range(0, n, epp)]
    assert len(slices) == len(GS)
    runs = {}
    for log_std in (-100.0, -3.0):
        nets = [policy(od, g, log_std) for g in GS]
        flat, num = _pack_wide(nets, od)
        runs[log_std] = _Rollout(_lanes_env(o, m, r, "fast", n=n), 1, obs).population(flat, epp)
        assert bool((flat[:, num:] == SENTINEL).all()), "behind a policy's parameters within its stride"
    run = runs[-100.0]
    assert torch.equal(run.obs_buf[0].cpu().view(torch.int32), obs.view(torch.int32)), "obs_buf[0] is the set"
    after = run.env.obs.cpu()
    for q, (g, sl) in enumerate(zip(GS, slices)):
        case = f"od {od} member {q} (g {g})"
        ref = yardstick(nets[q], obs[sl])
        _mean_and_value_held("rollout_population", case, run.act_buf[0, sl], run.val_buf[0, sl], ref)
        _logp_held("rollout_population", case, runs[-3.0].logp_buf[0, sl], runs[-3.0].act_buf[0, sl], ref, -3.0)
        _model_figures("rollout_population", case, nets[q], obs[sl], ref)
        # last_val: the rows are the env's own after one step from a CONST reset -- at most 64 of them, almost one
        # point.  Where torch32 is within half an f32 ulp of float64 on every one of them (err32 < 2^-24 of the output's
        # scale: correctly rounded, the least error an fp32 evaluation can show) the draw says nothing about an fp32
        # evaluation's error, the bar falls to 3.9 units of 2^-22 and the design itself (8e-7 on the value at g = 1, from
        # sum |-2 w| = 17 at an output below 1) meets it only by chance: DESIGN.md "Policy forward against float64".
        # The yardstick is then torch32's error for the same policy over its 1,094-row mixed set.  (od 3, g = 1 only.)
        last = yardstick(nets[q], after[sl])
        e32 = last["err32_val"]
        if e32 < 2.0 ** -24 * max(1.0, float(last["val64"].abs().max())):
            print(f"F64 | rollout_population | {case} | last_val rows alone | torch32 {e32:.3e} | bar {last['bar_val']:.3e}")
            e32 = reference(od, g, "mixed")["err32_val"]
        _held("rollout_population", case, "last_val", err(run.last_val[sl].cpu(), last["val64"]), e32,
              bar(e32, last["val64"]))
        _model_figures("rollout_population last_val", case, nets[q], after[sl], last)


@pytest.mark.parametrize("od", [3, 5])
def test_the_inference_error_leaves_the_first_update_unclipped(od):
    from b747_rl_ctrl_amd import _lib
    T, n, g, log_std, clip = 14, 70, 3, -3.0, 0.2
    o, m, r = CONFIG[od]
    net = policy(od, g, log_std)
    run = _Rollout(_lanes_env(o, m, r, "fast", n=n), T).single("b747_ppo_rollout_lanes", _packed(net, od))
    rows = T * n
    obs, act, logp = run.obs_buf[:T].reshape(rows, od), run.act_buf[:T].reshape(rows), run.logp_buf[:T].reshape(rows)
    ref, case = yardstick(net, obs), f"od {od} g {g} T {T} n {n}"
    _held("training", case, "value", err(run.val_buf[:T].reshape(rows).cpu(), ref["val64"]), ref["err32_val"],
          ref["bar_val"])
    _model_figures("training", case, net, obs, ref)
    diff, bound = _logp_held("training", case, logp, act, ref, log_std)
    delta = float(bound.max())
    assert delta < 0.5 * clip, f"delta {delta:.3e}: the check says nothing"
    gen = torch.Generator().manual_seed(NOISE_SEED + od)
    adv, ret = (0.3 + 1.5 * torch.randn(rows, generator=gen)).to(_dev()), torch.randn(rows, generator=gen).to(_dev())
    L = _lib.lib()
    theta = net.flat_params().to(_dev()).contiguous()
    ws = torch.empty(int(L.b747_ppo_update_workspace(od)), dtype=torch.uint8, device=_dev())
    grad, stats = torch.full((theta.numel(),), float("nan"), device=_dev()), torch.full((8,), float("nan"), device=_dev())
    idx = torch.arange(rows, dtype=torch.int64, device=_dev())
    _lib.check(L.b747_ppo_grad(_p(theta), od, _p(obs), _p(act), _p(logp), _p(adv), _p(ret), _p(idx), rows, clip, 0.0,
                               0.5, _p(ws), _p(grad), _p(stats), _stream()), "b747_ppo_grad")
    torch.cuda.synchronize()
    kl_bound = 0.5 * delta * delta * (1.0 + delta)
    print(f"F64 | training | {case} | update | max logp err {float(diff.max()):.3e} | delta {delta:.3e} | "
          f"clip fraction {float(stats[3]):.3e} | approx_kl {float(stats[4]):.3e} | bound {kl_bound:.3e}")
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(grad).all())
    assert float(stats[3]) == 0.0, f"clip fraction {float(stats[3])}"
    assert float(stats[4]) <= kl_bound, f"approx_kl {float(stats[4]):.3e} > {kl_bound:.3e}"
