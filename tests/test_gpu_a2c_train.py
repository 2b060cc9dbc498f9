"""ppo.A2C on the device: the fused update against the default torch path and a fp64 replay, the
one-graph iteration against the plain one, ControlTest on an A2C learner, and the one-wave rollout kernel under it.
64 envs x 5 steps of PID_LIKE; yardstick and margins of tests/test_gpu_ppo_update.py
(test_train_end_to_end_against_the_default_path_and_fp64): max |x - x64| / max |x64| per parameter tensor, relative error
per statistic, the fused path at most MARGIN = 4 times the default fp32 path's error plus a floor of 1e-7."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 4.0, 1e-7
N, T, ITERATIONS = 64, 5, 3
PARAM_NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "wa", "ba", "wv", "bv", "log_std")
ROLLOUT_BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf")
OPTIMIZERS = {"rmsprop": {}, "rmsprop_tf": {"rms_eps": 1e-9}, "adam": {}}


def _env(n=N, seed=3, **kw):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, seed=seed, **kw)


def _cfg(optimizer="rmsprop", **kw):
    from b747_rl_ctrl_amd.ppo import A2CConfig
    return A2CConfig(optimizer=optimizer, **(OPTIMIZERS[optimizer] | kw))


def _err(x, x64):
    x64 = x64.double()
    return float((x.double() - x64).abs().max() / x64.abs().max())


class _Fp64:
    """A2C.train in fp64 torch on a learner's rollout buffers: the policy, the optimiser the configuration names (the
    TF-like one from its formula: state at ones, epsilon inside the root) and the statistics of one step"""

    def __init__(self, a2c):
        from b747_rl_ctrl_amd.ppo import ActorCritic
        self.a2c, c = a2c, a2c.cfg
        self.pol = ActorCritic(a2c.env.obs_dim).to(a2c.env.device).double()
        self.pol.load_state_dict({k: v.double() for k, v in a2c.policy.state_dict().items()})
        prm = list(self.pol.parameters())
        if c.optimizer == "rmsprop":
            self.opt = torch.optim.RMSprop(prm, lr=c.learning_rate, alpha=c.rms_alpha, eps=c.rms_eps)
        elif c.optimizer == "adam":
            self.opt = torch.optim.Adam(prm, lr=c.learning_rate, eps=1e-5)
        else:
            self.opt, self.sq = None, [torch.ones_like(p) for p in prm]

    def step(self):
        a2c, c, pol = self.a2c, self.a2c.cfg, self.pol
        n_rows = T * a2c.env.n
        obs, act, adv, ret, val = (b[:T].reshape(n_rows, *b.shape[2:]).double()
                                   for b in (a2c.obs_buf, a2c.act_buf, a2c.adv_buf, a2c.ret_buf, a2c.val_buf))
        mean, value = pol(obs)
        logp = pol.log_prob(mean, act)
        a = (adv - adv.mean()) / (adv.std() + 1e-8) if c.normalize_advantage else adv
        pl, vf, ent = -(a * logp).mean(), ((ret - value) ** 2).mean(), -pol.entropy()
        loss = pl + c.ent_coef * ent + c.vf_coef * vf
        pol.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), c.max_grad_norm)
        if self.opt is not None:
            self.opt.step()
        else:
            with torch.no_grad():
                for p, sq in zip(pol.parameters(), self.sq):
                    sq.mul_(c.rms_alpha).addcmul_(p.grad, p.grad, value=1 - c.rms_alpha)
                    p.sub_(c.learning_rate * p.grad / torch.sqrt(sq + c.rms_eps))
        pl, vf, ent, loss = pl.detach(), vf.detach(), ent.detach(), loss.detach()
        return {"policy_loss": float(pl), "value_loss": float(vf), "entropy_loss": float(ent), "loss": float(loss),
                "explained_variance": float(1 - (ret - val).var(unbiased=False) / ret.var(unbiased=False)),
                "std": float(pol.log_std.detach().exp().mean()),
                "pg_term_scale": float((a * logp).detach().abs().mean())}


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
def test_train_end_to_end_against_the_default_path_and_fp64(optimizer):
    """Three iterations.  The fused learner flies the rollouts; the default learner and the fp64 replay take its buffers,
    so that all three paths see the same data and differ in their own arithmetic only.
    Measured on an MI355X (error against fp64 after the three steps): the fused path's parameter tensors 4e-9 to 3.8e-6,
    the default path's 4e-9 to 4.9e-6, the fused error 0.01 to 1.5 times the default's per tensor; the statistics 3e-10
    to 8e-8 for both but explained_variance (1e-4 to 2e-3, the same on both paths: the fp32 rollout buffers')."""
    from b747_rl_ctrl_amd.ppo import A2C
    cfg = _cfg(optimizer, ent_coef=0.01)
    pf = A2C(_env(), cfg, seed=5, fused_update=True)
    pd = A2C(_env(), cfg, seed=5)
    assert pf.fused_update and not pd.fused_update
    assert all(torch.equal(v, pd.policy.state_dict()[k]) for k, v in pf.policy.state_dict().items())
    r64 = _Fp64(pf)
    pf.last_obs.copy_(pf.env.reset())
    for it in range(ITERATIONS):
        pf.collect_rollouts(T)
        pf.compute_gae(T)
        for name in ROLLOUT_BUFS:                      # the same rollout through all three paths
            getattr(pd, name).copy_(getattr(pf, name))
        s64 = r64.step()
        sf, sd = pf.train(T), pd.train(T)
        assert set(sf) == set(sd) == set(s64)
        assert {"policy_loss", "value_loss", "entropy_loss", "explained_variance", "std", "loss"} <= set(sf)
    # every other method sees the new policy: the modules hold the flat master copy
    assert torch.equal(pf.policy.flat_params(), pf.flat[:pf.n_params])
    assert int(pf.upd_t) == ITERATIONS and not pf.opt.state
    assert hasattr(pf, "upd_sq") != (optimizer == "adam") and hasattr(pf, "upd_m") == (optimizer == "adam")
    bad = []
    for name, xf, xd, x64 in zip(PARAM_NAMES, pf.policy.flat_param_list(), pd.policy.flat_param_list(),
                                 r64.pol.flat_param_list()):
        e_f, e_d = _err(xf.detach(), x64.detach()), _err(xd.detach(), x64.detach())
        print(f"{optimizer} param {name:8s} fused {e_f:.3e} default {e_d:.3e}")
        if not e_f <= MARGIN * e_d + FLOOR:
            bad.append((name, e_f, e_d))
    for name in sorted(s64):                           # the last iteration's statistics
        assert math.isfinite(sf[name]), name
        if s64[name] == 0.0:
            assert sf[name] == 0.0, name
            continue
        e_f, e_d = abs(sf[name] - s64[name]) / abs(s64[name]), abs(sd[name] - s64[name]) / abs(s64[name])
        print(f"{optimizer} stat {name:22s} fused {e_f:.3e} default {e_d:.3e}")
        if not e_f <= MARGIN * e_d + FLOOR:
            bad.append((name, e_f, e_d))
    assert not bad, bad


@pytest.mark.parametrize("optimizer", ["rmsprop_tf", "adam"])
def test_learn_with_one_graph_per_iteration_gives_the_same_bits(optimizer):
    from b747_rl_ctrl_amd.ppo import A2C
    out = []
    for use_graph in (False, True):
        a2c = A2C(_env(), _cfg(optimizer, normalize_advantage=True, ent_coef=0.01), seed=7, fused_update=True,
                  rollout_kernel="lanes")
        assert a2c.rollout_kernel == "lanes"
        hist = a2c.learn(ITERATIONS, use_graph=use_graph)
        torch.cuda.synchronize()
        state = [a2c.upd_m, a2c.upd_v] if optimizer == "adam" else [a2c.upd_sq]
        out.append((hist, [a2c.flat, a2c.upd_t, a2c.step_base, a2c.policy.flat_params()] + state))
        assert int(a2c.upd_t) == ITERATIONS and len(hist) == ITERATIONS
        assert all(math.isfinite(v) for h in hist for v in h.values())
    (h0, t0), (h1, t1) = out
    assert all(torch.equal(a, b) for a, b in zip(t0, t1))
    assert h0 == h1
    assert not torch.equal(t0[0], A2C(_env(), _cfg(optimizer), seed=7).flat)        # (it did train)
    with pytest.raises(ValueError, match="fused_update"):
        A2C(_env(), _cfg(optimizer), seed=7).learn(1, use_graph=True)


def test_control_test_on_an_a2c_learner():
    from b747_rl_ctrl_amd.ppo import A2C, ControlTest
    a2c = A2C(_env(), _cfg("rmsprop_tf"), seed=2, fused_update=True, rollout_kernel="lanes")
    refs = [math.radians(5.0), math.radians(-5.0)]
    ct = ControlTest(a2c, refs, log_interval=T, window_length=3, tk=1.0)
    ct.evaluate()
    torch.cuda.synchronize()
    assert ct.evaluations == 1 and ct.count.tolist() == [1]
    assert torch.isfinite(ct.last).all() and torch.isfinite(ct.window_mean).all()
    hist = a2c.learn(2, control_test=ct)               # log_interval = T: one evaluation before each iteration
    assert ct.evaluations == 3 and ct.count.tolist() == [3]
    for h in hist:
        assert {"transfer_settling_time", "transfer_overshoot", "transfer_quality"} <= set(h)
        assert all(torch.isfinite(h[k]).all() for k in ("transfer_settling_time", "transfer_overshoot", "transfer_quality"))
    # and inside the one-graph form: the evaluations stay outside the capture
    hist = a2c.learn(2, control_test=ct, use_graph=True)
    assert ct.evaluations == 5 and "transfer_quality" in hist[-1]


def test_the_lanes_rollout_collects_the_two_launch_buffers_in_faithful():
    from b747_rl_ctrl_amd.ppo import A2C
    p1 = A2C(_env(variant="faithful", sample_time=0.05), _cfg(), seed=1, rollout_kernel="lanes")
    p2 = A2C(_env(variant="faithful", sample_time=0.05), _cfg(), seed=1, rollout_kernel=False)
    assert p1.rollout_kernel == "lanes" and p2.rollout_kernel is False
    for _ in range(2):                                 # the second rollout starts mid-episode, with fresh noise
        p1.collect_rollouts(T, use_graph=False)
        p2.collect_rollouts(T, use_graph=False)
        torch.cuda.synchronize()
        for name in ROLLOUT_BUFS[:6]:
            a, b = getattr(p1, name), getattr(p2, name)
            same = (a == b) | (a.isnan() & b.isnan()) if a.is_floating_point() else a == b
            assert bool(same.all()), name
    assert int(p1.step_base) == 2 * T == int(p2.step_base)
    assert bool(p1.done_buf.any())                     # tk 0.3 at sample_time 0.05: episodes end in the second rollout
