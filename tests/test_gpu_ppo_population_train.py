"""Population training (ppo.PopulationPPO, b747_ppo_epoch_population) against what the project already
has for ONE learner, composed per member: b747_ppo_rollout_lanes on the member's own envs, the b747_policy_act
bootstrap value, b747_ppo_gae and b747_ppo_epoch.  The population calls issue the same kernels on the same numbers in
the same order per member, so everything is compared with torch.equal -- no tolerance.

Shapes: P = 3 members of 64 envs, T = 14 steps (896 rows per member, 2,688 in the shared buffers), batch_size 256: four
minibatches per member and epoch, the last one partial (128 rows), two epochs.  tk 0.3 at sample_time 0.05: 6-step
episodes, so the rollouts hold episode ends and auto-resets."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

P, EPP, T, BATCH, EPOCHS = 3, 64, 14, 256, 2
N = P * EPP
SEED, ENV_SEED = 1, 3
SEEDS = [5, 6, 7]
LRS = [3e-4, 1e-3, 1e-4]
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3}]


def _env(n, offset=0, variant="faithful", rew_config=None):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    env = BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, sample_time=0.05,
                             seed=ENV_SEED, env_offset=offset, variant=variant)
    if rew_config is not None:
        env.set_rew_config(rew_config)
    return env


def _population(variant="faithful"):
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS, ent_coef=0.01)
    return PopulationPPO(_env(N, variant=variant), P, EPP, cfg, seeds=SEEDS, rew_configs=REW_CONFIGS,
                         learning_rates=LRS, seed=SEED)


def _order(epoch, T_, n, p):
    """the sample order of member p in an epoch, over the member's own rows t * n + j"""
    return torch.randperm(T_ * n, generator=torch.Generator().manual_seed(100 * epoch + p))


def test_the_epoch_call_is_the_per_member_loop_of_epoch_calls():
    from b747_rl_ctrl_amd import _lib
    L, ptr = _lib.lib(), lambda x: x.data_ptr()
    pp = _population("fast")
    pp.env.reset()
    pp.collect_rollouts(T)
    pp.compute_gae(T)
    c, od, n_rows = pp.cfg, pp.env.obs_dim, T * EPP
    n_mb = -(-n_rows // BATCH)
    assert n_mb == 4 and n_rows % BATCH == 128 and (P * n_rows) % BATCH != 1
    rows_of = pp.member_rows(T)
    assert torch.equal(rows_of[1, :2], torch.tensor([EPP, EPP + 1], device=rows_of.device)) and int(rows_of[2, EPP]) == N + 2 * EPP
    perms = [torch.stack([rows_of[p][_order(e, T, EPP, p).to(rows_of.device)] for p in range(P)]).contiguous()
             for e in range(EPOCHS)]
    bufs = (pp.obs_buf, pp.act_buf, pp.logp_buf, pp.adv_buf, pp.ret_buf)
    stream = torch.cuda.current_stream().cuda_stream

    def state():
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=pp.flat.device)
        return {"theta": pp.flat.clone(), "m": z(P, pp.n_params), "v": z(P, pp.n_params),
                "t": torch.zeros(P, dtype=torch.int64, device=pp.flat.device),
                "stats": torch.full((EPOCHS, P, n_mb, 8), float("nan"), device=pp.flat.device)}
    loop, call = state(), state()
    grad = torch.empty(pp.n_params, dtype=torch.float32, device=pp.flat.device)
    lr = (ctypes.c_double * P)(*LRS)
    for e in range(EPOCHS):
        for m in range(P):                                # the path without the new entry point
            _lib.check(L.b747_ppo_epoch(
                ptr(loop["theta"][m]), od, *(ptr(b) for b in bufs), ptr(perms[e][m]), n_rows, BATCH, c.clip_range,
                c.ent_coef, c.vf_coef, ptr(pp.upd_ws), ptr(grad), ptr(loop["m"][m]), ptr(loop["v"][m]),
                ptr(loop["t"][m:]), c.max_grad_norm, LRS[m], 0.9, 0.999, 1e-5, ptr(loop["stats"][e, m]), stream),
                "b747_ppo_epoch")
        _lib.check(L.b747_ppo_epoch_population(
            ptr(call["theta"]), P, pp.stride, od, *(ptr(b) for b in bufs), ptr(perms[e]), n_rows, BATCH, c.clip_range,
            c.ent_coef, c.vf_coef, ptr(pp.upd_ws), ptr(grad), ptr(call["m"]), ptr(call["v"]), ptr(call["t"]),
            c.max_grad_norm, lr, 0.9, 0.999, 1e-5, ptr(call["stats"][e]), stream), "b747_ppo_epoch_population")
    torch.cuda.synchronize()
    assert loop["t"].tolist() == [EPOCHS * n_mb] * P
    assert bool(torch.isfinite(loop["stats"]).all()) and bool(torch.isfinite(loop["theta"][:, :pp.n_params]).all())
    for m in range(P):
        assert not torch.equal(loop["theta"][m, :pp.n_params], pp.flat[m, :pp.n_params]), "the member was updated"
    for name in loop:
        assert torch.equal(loop[name], call[name]), \
            f"{name}: {int((loop[name] != call[name]).sum())} of {loop[name].numel()} entries differ"


class _Member:
    """one learner composed from the single-policy calls, on the member's own envs"""

    def __init__(self, p):
        from b747_rl_ctrl_amd import _lib
        from b747_rl_ctrl_amd.evaluate import packed_policy
        from b747_rl_ctrl_amd.ppo import ActorCritic
        self.p, self._lib, self.L = p, _lib, _lib.lib()
        self.env = _env(EPP, p * EPP, "faithful", REW_CONFIGS[p])
        dev, od = self.env.device, self.env.obs_dim
        torch.manual_seed(SEEDS[p])
        net = ActorCritic(od)
        self.n_params = net.flat_params().numel()
        self.flat = packed_policy(net, od, dev)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        self.obs_buf, self.act_buf = z(T, EPP, od), z(T, EPP, 1)
        self.logp_buf, self.val_buf, self.rew_buf = z(T, EPP), z(T, EPP), z(T, EPP)
        self.done_buf = z(T, EPP, dt=torch.bool)
        self.adv_buf, self.ret_buf, self.last_val = z(T, EPP), z(T, EPP), z(EPP)
        self.m, self.v, self.grad = z(self.n_params), z(self.n_params), z(self.n_params)
        self.t, self.step_base = z(1, dt=torch.int64), z(1, dt=torch.int64)
        self.ws = torch.empty(int(self.L.b747_ppo_update_workspace(od)), dtype=torch.uint8, device=dev)
        self.stats = z(-(-T * EPP // BATCH), 8)
        self.scratch = [z(EPP) for _ in range(3)]

    def iteration(self, cfg):
        env, L, chk, ptr = self.env, self.L, self._lib.check, lambda x: x.data_ptr()
        stream, od = torch.cuda.current_stream().cuda_stream, self.env.obs_dim
        b = env._batch()
        b.action = ptr(env.action)
        chk(L.b747_ppo_rollout_lanes(env._bref, env._cref, env._kref, ptr(self.flat), SEED, ptr(self.step_base), T,
                                     ptr(self.obs_buf), ptr(self.act_buf), ptr(self.logp_buf), ptr(self.val_buf),
                                     ptr(self.rew_buf), ptr(self.done_buf), -1.0, 1.0, stream), "b747_ppo_rollout_lanes")
        chk(L.b747_policy_act(ptr(self.flat), od, EPP, ptr(env.obs), None, SEED, None, 0, env.env_offset, None,
                              ptr(self.scratch[0]), ptr(self.scratch[1]), ptr(self.last_val), ptr(self.scratch[2]),
                              -1.0, 1.0, stream), "b747_policy_act")
        chk(L.b747_ppo_gae(ptr(self.rew_buf), ptr(self.val_buf), ptr(self.done_buf), ptr(self.last_val), T, EPP,
                           cfg.gamma, cfg.gae_lambda, ptr(self.adv_buf), ptr(self.ret_buf), stream), "b747_ppo_gae")
        for e in range(cfg.n_epochs):
            perm = _order(e, T, EPP, self.p).to(env.device).contiguous()
            chk(L.b747_ppo_epoch(ptr(self.flat), od, ptr(self.obs_buf), ptr(self.act_buf), ptr(self.logp_buf),
                                 ptr(self.adv_buf), ptr(self.ret_buf), ptr(perm), T * EPP, cfg.batch_size, cfg.clip_range,
                                 cfg.ent_coef, cfg.vf_coef, ptr(self.ws), ptr(self.grad), ptr(self.m), ptr(self.v),
                                 ptr(self.t), cfg.max_grad_norm, LRS[self.p], 0.9, 0.999, 1e-5, ptr(self.stats), stream),
                "b747_ppo_epoch")
        chk(L.b747_policy_pack(ptr(self.flat), od, stream), "b747_policy_pack")


def test_learn_gives_the_bits_of_separate_learners():
    pp = _population("faithful")
    initial = pp.flat[:, :pp.n_params].clone()
    hist = pp.learn(2, T, minibatch_order=_order)
    members = [_Member(p) for p in range(P)]
    for mem in members:
        assert torch.equal(initial[mem.p], mem.flat[:pp.n_params]), "the initial policy PPO(seed=seeds[p]) builds"
        mem.env.reset()
    for _ in range(2):
        for mem in members:
            mem.iteration(pp.cfg)
    torch.cuda.synchronize()
    assert int(pp.step_base) == 2 * T and pp.upd_t.tolist() == [2 * EPOCHS * 4] * P
    for mem in members:
        p = mem.p
        sl = slice(p * EPP, (p + 1) * EPP)
        # (the last rollout and its advantages first: a difference there names the stage)
        for name in ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf"):
            assert torch.equal(getattr(pp, name)[:T, sl], getattr(mem, name)), f"member {p}: {name}"
        assert torch.equal(pp.last_val[sl], mem.last_val), f"member {p}: last_val"
        assert torch.equal(pp.upd_m[p], mem.m) and torch.equal(pp.upd_v[p], mem.v), f"member {p}: Adam moments"
        assert torch.equal(pp.flat[p, :pp.n_params], mem.flat[:pp.n_params]), f"member {p}: the flat parameters"
        assert torch.equal(pp.flat[p], mem.flat), f"member {p}: the packed sections"
        assert not torch.equal(pp.flat[p, :pp.n_params], initial[p]), f"member {p} did not learn"
    for a in range(P):
        for b in range(a + 1, P):
            assert not torch.equal(pp.flat[a, :pp.n_params], pp.flat[b, :pp.n_params])
    assert len(hist) == 2
    for h in hist:
        for k, v in h.items():
            assert tuple(v.shape) == (P,) and (k == "explained_variance" or bool(torch.isfinite(v).all())), (k, v)
    keys = {"entropy_loss", "policy_gradient_loss", "value_loss", "approx_kl", "clip_fraction", "loss",
            "explained_variance", "std", "pg_term_scale", "kl_term_scale", "policy_loss", "mean_reward"}
    assert set(hist[0]) == keys


def test_step_tests_ranks_the_members_as_population_step_tests_does():
    from b747_rl_ctrl_amd.evaluate import population_step_tests
    pp = _population("fast")
    pp.learn(1, T)
    refs = [math.radians(5), math.radians(-5), math.radians(10), math.radians(-10)]
    out = pp.step_tests(refs, tk=2.0)
    e = pp.env
    ref = population_step_tests([pp.member(p) for p in range(P)], refs, tk=2.0, observation_type=e.observation_type,
                                reward_type=e.reward_type, ctrl_mode=e.ctrl_mode, norm_obs=e.norm_obs,
                                norm_act=e.norm_act, sample_time=e.sample_time, device=e.device, action_max=e.action_max,
                                vartheta_max=e.vartheta_max, use_limiter=e.use_limiter, variant="fast")
    for k in ("mean_quality", "mean_overshoot", "mean_settling_time"):
        assert tuple(out[k].shape) == (P,)
        same = (out[k] == ref[k]) | (out[k].isnan() & ref[k].isnan())
        assert bool(same.all()), (k, out[k], ref[k])
    assert tuple(out["quality"].shape) == (P, len(refs)) and int(out["best"]) == int(ref["best"])
    assert bool(torch.isfinite(out["mean_quality"]).all())
