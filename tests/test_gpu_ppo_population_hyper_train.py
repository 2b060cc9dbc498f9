"""Population training with per-member hyper-parameters (ppo.PopulationPPO(hyper=...), b747_ppo_gae_population,
b747_ppo_epoch_population_hyper, b747_ppo_epoch_batched_hyper) against what the project has for ONE
learner, composed per member with that member's values: b747_ppo_rollout_lanes on the member's own envs, the
b747_policy_act bootstrap value, b747_ppo_gae and b747_ppo_epoch (as tests/test_gpu_ppo_population_train.py).  The
population calls issue the same operations on the same numbers in the same order per member, so everything is compared
with torch.equal -- no tolerance.

Shapes: P = 3 members of 64 envs, T = 14 steps (896 rows per member), batch_size 256: four minibatches per member and
epoch, the last one partial (128 rows), two epochs, two iterations.  tk 0.3 at sample_time 0.05: 6-step episodes, so the
rollouts hold episode ends and auto-resets."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

P, EPP, T, BATCH, EPOCHS = 3, 64, 14, 256, 2
N = P * EPP
SEED, ENV_SEED = 1, 3
SEEDS = [5, 6, 7]
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3}]
HYPER = [dict(learning_rate=3e-4, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, gamma=0.99,
              gae_lambda=0.95),
         dict(learning_rate=1e-3, clip_range=0.1, ent_coef=0.0, vf_coef=0.25, max_grad_norm=0.05, gamma=0.9,
              gae_lambda=0.6),
         dict(learning_rate=1e-4, clip_range=0.3, ent_coef=0.005, vf_coef=0.6, max_grad_norm=10.0, gamma=0.7,
              gae_lambda=1.0)]
NEW_ROW_1 = dict(learning_rate=5e-4, clip_range=0.15, gamma=0.95)      # set_hyper(1, ...): a column of each kernel
BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf")
STATE = ("flat", "upd_m", "upd_v", "upd_t")


def _env(n, offset=0, rew_config=None):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    env = BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, sample_time=0.05,
                             seed=ENV_SEED, env_offset=offset, variant="faithful")
    if rew_config is not None:
        env.set_rew_config(rew_config)
    return env


def _cfg():
    from b747_rl_ctrl_amd.ppo import PPOConfig
    return PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS, ent_coef=0.01)


def _population(hyper, batched, **kw):
    from b747_rl_ctrl_amd.ppo import PopulationPPO
    return PopulationPPO(_env(N), P, EPP, _cfg(), seeds=SEEDS, rew_configs=REW_CONFIGS, seed=SEED,
                         batched_update=batched, hyper=hyper, **kw)


def _order(epoch, T_, n, p):
    """the sample order of member p in an epoch, over the member's own rows t * n + j"""
    return torch.randperm(T_ * n, generator=torch.Generator().manual_seed(100 * epoch + p))


def _iteration(pp):
    pp.collect_rollouts(T)
    pp.compute_gae(T)
    return pp.train(T, _order)


class _Member:
    """one learner composed from the single-policy calls, on the member's own envs, with the member's own values"""

    def __init__(self, p):
        from b747_rl_ctrl_amd import _lib
        from b747_rl_ctrl_amd.evaluate import packed_policy
        from b747_rl_ctrl_amd.ppo import ActorCritic
        self.p, self.h, self._lib, self.L = p, HYPER[p], _lib, _lib.lib()
        self.env = _env(EPP, p * EPP, REW_CONFIGS[p])
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

    def iteration(self):
        env, L, chk, ptr, h = self.env, self.L, self._lib.check, (lambda x: x.data_ptr()), self.h
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
                           h["gamma"], h["gae_lambda"], ptr(self.adv_buf), ptr(self.ret_buf), stream), "b747_ppo_gae")
        for e in range(EPOCHS):
            perm = _order(e, T, EPP, self.p).to(env.device).contiguous()
            chk(L.b747_ppo_epoch(ptr(self.flat), od, ptr(self.obs_buf), ptr(self.act_buf), ptr(self.logp_buf),
                                 ptr(self.adv_buf), ptr(self.ret_buf), ptr(perm), T * EPP, BATCH, h["clip_range"],
                                 h["ent_coef"], h["vf_coef"], ptr(self.ws), ptr(self.grad), ptr(self.m), ptr(self.v),
                                 ptr(self.t), h["max_grad_norm"], h["learning_rate"], 0.9, 0.999, 1e-5, ptr(self.stats),
                                 stream), "b747_ppo_epoch")
        chk(L.b747_policy_pack(ptr(self.flat), od, stream), "b747_policy_pack")


@functools.lru_cache(maxsize=None)
def _separate_learners():
    """two iterations of the three learners: computed once, shared, never modified"""
    members = [_Member(p) for p in range(P)]
    initial = [mem.flat.clone() for mem in members]
    for mem in members:
        mem.env.reset()
    for _ in range(2):
        for mem in members:
            mem.iteration()
    torch.cuda.synchronize()
    return members, initial


@pytest.mark.parametrize("batched", [False, True])
def test_learn_gives_the_bits_of_separate_learners_with_each_members_values(batched):
    from b747_rl_ctrl_amd.ppo import hyper_table
    members, initial = _separate_learners()
    pp = _population(HYPER, batched)
    assert torch.equal(pp.hyper, hyper_table(_cfg(), P, HYPER)) and torch.equal(pp.hyper_dev.cpu(), pp.hyper)
    assert pp.learning_rates == [h["learning_rate"] for h in HYPER]
    for mem in members:
        assert torch.equal(pp.flat[mem.p, :pp.n_params], initial[mem.p][:pp.n_params]), \
            "the initial policy PPO(seed=seeds[p]) builds"
    hist = pp.learn(2, T, minibatch_order=_order)
    torch.cuda.synchronize()
    assert int(pp.step_base) == 2 * T and pp.upd_t.tolist() == [2 * EPOCHS * 4] * P
    for mem in members:
        p = mem.p
        sl = slice(p * EPP, (p + 1) * EPP)
        # (the last rollout and its advantages first: a difference there names the stage)
        for name in BUFS:
            assert torch.equal(getattr(pp, name)[:T, sl], getattr(mem, name)), f"member {p}: {name}"
        assert torch.equal(pp.last_val[sl], mem.last_val), f"member {p}: last_val"
        assert torch.equal(pp.upd_m[p], mem.m) and torch.equal(pp.upd_v[p], mem.v), f"member {p}: Adam moments"
        assert int(pp.upd_t[p]) == int(mem.t), f"member {p}: Adam step count"
        assert torch.equal(pp.flat[p, :pp.n_params], mem.flat[:pp.n_params]), f"member {p}: the flat parameters"
        assert torch.equal(pp.flat[p], mem.flat), f"member {p}: the packed sections"
        assert not torch.equal(pp.flat[p, :pp.n_params], initial[p][:pp.n_params]), f"member {p} did not learn"
    assert len(hist) == 2 and all(tuple(v.shape) == (P,) for h in hist for v in h.values())


@pytest.mark.parametrize("batched", [False, True])
def test_rows_that_all_equal_cfg_give_the_bits_of_the_population_without_a_table(batched):
    lrs = [3e-4, 1e-3, 1e-4]
    plain = _population(None, batched, learning_rates=lrs)
    table = _population([{}, {}, {}], batched, learning_rates=lrs)
    assert plain.hyper is None and plain.hyper_dev is None
    c = _cfg()
    assert table.hyper[:, 1:7].tolist() == [[c.clip_range, c.ent_coef, c.vf_coef, c.max_grad_norm, c.gamma,
                                             c.gae_lambda]] * P and table.hyper[:, 0].tolist() == lrs
    for pp in (plain, table):
        pp.learn(2, T, minibatch_order=_order)
    torch.cuda.synchronize()
    for name in BUFS + ("last_val",) + STATE:
        assert torch.equal(getattr(plain, name), getattr(table, name)), name
    assert plain.upd_t.tolist() == [2 * EPOCHS * 4] * P


@pytest.mark.parametrize("batched", [False, True])
def test_set_hyper_between_two_iterations_is_a_population_built_with_the_new_row(batched):
    """A is built with HYPER and gets member 1's new values after its first iteration; B is built with the new row.
    The first rollout does not depend on the table (the initial policies fly it), so after it the two envs are in the
    same state; B then takes A's learner state, and the second iterations must agree bit for bit."""
    a = _population(HYPER, batched)
    b = _population([HYPER[0], HYPER[1] | NEW_ROW_1, HYPER[2]], batched)
    for pp in (a, b):
        pp.env.reset()
        _iteration(pp)
    for name in BUFS[:6]:
        assert torch.equal(getattr(a, name), getattr(b, name)), name            # the same first rollout
    assert not torch.equal(a.adv_buf[:, EPP:2 * EPP], b.adv_buf[:, EPP:2 * EPP])  # (member 1's gamma differs)
    assert torch.equal(a.adv_buf[:, :EPP], b.adv_buf[:, :EPP]) and torch.equal(a.flat[0], b.flat[0])
    assert not torch.equal(a.flat[1], b.flat[1])
    for name in STATE:
        getattr(b, name).copy_(getattr(a, name))
    row0, rows_dev = a.hyper[0].clone(), a.hyper_dev.clone()
    a.set_hyper(1, **NEW_ROW_1)
    assert torch.equal(a.hyper, b.hyper) and torch.equal(a.hyper_dev.cpu(), b.hyper) and torch.equal(a.hyper[0], row0)
    assert torch.equal(a.hyper_dev[0], rows_dev[0]) and torch.equal(a.hyper_dev[2], rows_dev[2])
    assert a.learning_rates == b.learning_rates and a.learning_rates[1] == NEW_ROW_1["learning_rate"]
    for pp in (a, b):
        _iteration(pp)
    torch.cuda.synchronize()
    for name in BUFS + ("last_val",) + STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.upd_t.tolist() == [2 * EPOCHS * 4] * P


def test_set_hyper_validates_before_it_writes():
    pp = _population(HYPER, True)
    keep, keep_dev = pp.hyper.clone(), pp.hyper_dev.clone()
    for kw, word in ((dict(gamma=1.5), "gamma"), (dict(clip_range=0.1, learning_rate=0.0), "learning_rate"),
                     (dict(n_steps=8), "n_steps"), (dict(ent_coef=float("nan")), "ent_coef")):
        with pytest.raises(ValueError, match=word):
            pp.set_hyper(1, **kw)
    with pytest.raises(ValueError, match="member 3"):
        pp.set_hyper(3, gamma=0.5)
    assert torch.equal(pp.hyper, keep) and torch.equal(pp.hyper_dev, keep_dev)


def test_copy_member_makes_the_target_the_source_and_leaves_the_others_alone():
    pp = _population(HYPER, True)
    pp.learn(1, T, minibatch_order=_order)
    before = {name: getattr(pp, name).clone() for name in STATE + ("hyper", "hyper_dev")}
    assert not torch.equal(pp.flat[0], pp.flat[2]) and not torch.equal(pp.upd_m[0], pp.upd_m[2])
    pp.copy_member(0, 2, hyper=False)
    torch.cuda.synchronize()
    for name in STATE:
        x = getattr(pp, name)
        assert torch.equal(x[2], before[name][0]) and torch.equal(x[:2], before[name][:2]), name
    assert torch.equal(pp.hyper, before["hyper"]) and torch.equal(pp.hyper_dev, before["hyper_dev"])
    pp.copy_member(1, 1)                                  # (onto itself: nothing)
    pp.flat[2].fill_(0.0)
    pp.copy_member(0, 2)
    torch.cuda.synchronize()
    for name in STATE + ("hyper", "hyper_dev"):
        x = getattr(pp, name)
        assert torch.equal(x[2], before[name][0]) and torch.equal(x[:2], before[name][:2]), name
    assert pp.learning_rates == [HYPER[0]["learning_rate"], HYPER[1]["learning_rate"], HYPER[0]["learning_rate"]]
    with pytest.raises(ValueError, match="member 3"):
        pp.copy_member(0, 3)
    # the twins stay twins only as far as their envs and reward constants let them: they train on
    _iteration(pp)
    torch.cuda.synchronize()
    assert pp.upd_t.tolist() == [2 * EPOCHS * 4] * P and bool(torch.isfinite(pp.flat[:, :pp.n_params]).all())


def test_the_helpers_need_a_table():
    pp = _population(None, False)
    with pytest.raises(ValueError, match="hyper=None"):
        pp.set_hyper(0, gamma=0.9)
    with pytest.raises(ValueError, match="hyper=None"):
        pp.copy_member(0, 1)
    with pytest.raises(ValueError, match="gamma"):
        _population([{"gamma": 2.0}, {}, {}], False)
