"""ppo.PopulationA2C against what the project has for ONE A2C learner, composed per member with that
member's values (as tests/test_gpu_ppo_population_hyper_train.py): b747_ppo_rollout_lanes on the member's own envs
(env_offset), the b747_policy_act bootstrap value, b747_ppo_gae, b747_a2c_update with idx = NULL and b747_policy_pack.
The population calls issue the same operations on the same numbers in the same order per member, so everything is
compared with torch.equal -- no tolerance.

Shapes: P = 3 members of 64 envs, T = 5 steps (320 rows per member, one gradient step), two iterations.  tk 0.3 at
sample_time 0.05: 6-step episodes, so the second rollout holds episode ends and auto-resets.  The three optimisers are
spread over the members."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

P, EPP, T = 3, 64, 5
N = P * EPP
SEED, ENV_SEED = 1, 3
SEEDS = [5, 6, 7]
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3}]
HYPER = [dict(learning_rate=7e-4, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, gamma=0.99, gae_lambda=1.0,
              optimizer="rmsprop_tf"),
         dict(learning_rate=1e-3, ent_coef=0.0, vf_coef=0.25, max_grad_norm=0.05, gamma=0.9, gae_lambda=0.6,
              optimizer="adam"),
         dict(learning_rate=3e-4, ent_coef=0.005, vf_coef=0.6, max_grad_norm=10.0, gamma=0.7, gae_lambda=0.95,
              optimizer="rmsprop")]
NEW_ROW_1 = dict(learning_rate=5e-4, vf_coef=0.4, gamma=0.95)      # set_hyper(1, ...): a column of each kernel
BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf")
STATE = ("flat", "upd_s0", "upd_s1", "upd_t")
REFS = [math.radians(v) for v in (5.0, -5.0)]
LOG_KEYS = ("policy_loss", "value_loss", "entropy_loss", "loss", "explained_variance", "std", "pg_term_scale",
            "mean_reward")


def _env(n, offset=0, rew_config=None):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    env = BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, sample_time=0.05,
                             seed=ENV_SEED, env_offset=offset, variant="faithful")
    if rew_config is not None:
        env.set_rew_config(rew_config)
    return env


def _cfg(**kw):
    from b747_rl_ctrl_amd.ppo import A2CConfig
    return A2CConfig.reference(n_steps=T, normalize_advantage=True, rms_eps=1e-7, **kw)


def _population(hyper=HYPER, **kw):
    from b747_rl_ctrl_amd import PopulationA2C
    return PopulationA2C(_env(N), P, EPP, _cfg(), seeds=SEEDS, rew_configs=REW_CONFIGS, seed=SEED, hyper=hyper, **kw)


def _same(x, y):
    """two log values: the same bits, NaN equal to NaN"""
    return torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0))


def _same_history(a, b):
    return len(a) == len(b) and all(sorted(x) == sorted(y) and all(_same(x[k], y[k]) for k in x) for x, y in zip(a, b))


class _Member:
    """one A2C learner composed from the single-policy calls, on the member's own envs, with the member's own values"""

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
        self.s0 = torch.full((self.n_params,), 1.0 if self.h["optimizer"] == "rmsprop_tf" else 0.0, device=dev)
        self.s1, self.grad = z(self.n_params), z(self.n_params)
        self.t, self.step_base = z(1, dt=torch.int64), z(1, dt=torch.int64)
        self.ws = torch.empty(int(self.L.b747_ppo_update_workspace(od)), dtype=torch.uint8, device=dev)
        self.stats = z(8)
        self.scratch = [z(EPP) for _ in range(3)]

    def iteration(self):
        from b747_rl_ctrl_amd.ppo import A2C_OPTIMIZERS
        env, L, chk, ptr, h, c = self.env, self.L, self._lib.check, (lambda x: x.data_ptr()), self.h, _cfg()
        stream, od = torch.cuda.current_stream().cuda_stream, self.env.obs_dim
        adam = h["optimizer"] == "adam"
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
        chk(L.b747_a2c_update(ptr(self.flat), od, ptr(self.obs_buf), ptr(self.act_buf), ptr(self.adv_buf),
                              ptr(self.ret_buf), None, T * EPP, int(c.normalize_advantage), h["ent_coef"], h["vf_coef"],
                              ptr(self.ws), ptr(self.grad), ptr(self.stats), A2C_OPTIMIZERS.index(h["optimizer"]),
                              ptr(self.s0), ptr(self.s1) if adam else None, ptr(self.t), h["max_grad_norm"],
                              h["learning_rate"], c.rms_alpha, 1e-5 if adam else c.rms_eps, stream), "b747_a2c_update")
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


@functools.lru_cache(maxsize=None)
def _plain_run():
    """learn(2, T) of the population with HYPER, no graph: (the population, its history); shared, never modified"""
    pp = _population()
    hist = pp.learn(2, T)
    torch.cuda.synchronize()
    return pp, hist


def test_learn_gives_the_bits_of_separate_learners_with_each_members_values():
    from b747_rl_ctrl_amd.ppo import PopulationPPO, a2c_hyper_table
    members, initial = _separate_learners()
    fresh = _population()
    assert isinstance(fresh, PopulationPPO)
    assert torch.equal(fresh.hyper, a2c_hyper_table(_cfg(), P, HYPER)) and torch.equal(fresh.hyper_dev.cpu(), fresh.hyper)
    assert fresh.optimizers == [h["optimizer"] for h in HYPER]
    assert fresh.learning_rates == [h["learning_rate"] for h in HYPER]
    assert bool((fresh.upd_s0[0] == 1).all()) and bool((fresh.upd_s0[1:] == 0).all()) and bool((fresh.upd_s1 == 0).all())
    for mem in members:
        assert torch.equal(fresh.flat[mem.p, :fresh.n_params], initial[mem.p][:fresh.n_params]), \
            "the initial policy A2C(seed=seeds[p]) builds"
    pp, hist = _plain_run()
    assert int(pp.step_base) == 2 * T and pp.upd_t.tolist() == [2] * P
    for mem in members:
        p = mem.p
        sl = slice(p * EPP, (p + 1) * EPP)
        # (the last rollout and its advantages first: a difference there names the stage)
        for name in BUFS:
            assert torch.equal(getattr(pp, name)[:T, sl], getattr(mem, name)), f"member {p}: {name}"
        assert torch.equal(pp.last_val[sl], mem.last_val), f"member {p}: last_val"
        assert torch.equal(pp.upd_s0[p], mem.s0) and torch.equal(pp.upd_s1[p], mem.s1), f"member {p}: optimiser state"
        assert int(pp.upd_t[p]) == int(mem.t) == 2, f"member {p}: step count"
        assert torch.equal(pp.stats[p], mem.stats), f"member {p}: the statistics row"
        assert torch.equal(pp.flat[p, :pp.n_params], mem.flat[:pp.n_params]), f"member {p}: the flat parameters"
        assert torch.equal(pp.flat[p], mem.flat), f"member {p}: the packed sections"
        assert not torch.equal(pp.flat[p, :pp.n_params], initial[p][:pp.n_params]), f"member {p} did not learn"
    assert bool(pp.done_buf[:T].any()), "the second rollout holds episode ends"
    assert len(hist) == 2 and all(sorted(h) == sorted(LOG_KEYS) for h in hist)
    assert all(tuple(v.shape) == (P,) for h in hist for v in h.values())
    assert all(bool(torch.isfinite(h[k]).all()) for h in hist for k in LOG_KEYS)
    assert torch.equal(hist[-1]["loss"], pp.stats[:, 7].double())


def test_a_graph_replay_per_iteration_gives_the_same_bits():
    plain, hist = _plain_run()
    graph = _population()
    hist_g = graph.learn(2, T, use_graph=True)
    torch.cuda.synchronize()
    for name in BUFS + ("last_val", "stats", "step_base") + STATE:
        assert torch.equal(getattr(plain, name), getattr(graph, name)), name
    assert _same_history(hist, hist_g)
    graph.learn(1, T, use_graph=True)            # (the captured graph serves the next learn())
    torch.cuda.synchronize()
    assert graph.upd_t.tolist() == [3] * P and bool(torch.isfinite(graph.flat[:, :graph.n_params]).all())


def test_no_table_is_a_table_whose_rows_all_equal_cfg():
    lrs = [3e-4, 1e-3, 1e-4]
    plain, table = _population(None, learning_rates=lrs), _population([{}, {}, {}], learning_rates=lrs)
    c = _cfg()
    assert plain.hyper is not None and torch.equal(plain.hyper, table.hyper) and torch.equal(plain.hyper_dev.cpu(), plain.hyper)
    assert plain.hyper[:, 1:].tolist() == [[0.0, c.ent_coef, c.vf_coef, c.max_grad_norm, c.gamma, c.gae_lambda, 2.0]] * P
    assert plain.hyper[:, 0].tolist() == lrs and bool((plain.upd_s0 == 1).all())
    for pp in (plain, table):
        pp.learn(2, T)
    torch.cuda.synchronize()
    for name in BUFS + ("last_val", "stats") + STATE:
        assert torch.equal(getattr(plain, name), getattr(table, name)), name
    assert plain.upd_t.tolist() == [2] * P and not torch.equal(plain.flat[0], plain.flat[1])


def _iteration(pp):
    pp.collect_rollouts(T)
    pp.compute_gae(T)
    return pp.train(T)


def test_set_hyper_between_two_iterations_is_a_population_built_with_the_new_row():
    """A is built with HYPER and gets member 1's new values after its first iteration; B is built with the new row.
    The first rollout does not depend on the table (the initial policies fly it), so after it the two envs are in the
    same state; B then takes A's learner state, and the second iterations must agree bit for bit."""
    a = _population()
    b = _population([HYPER[0], HYPER[1] | NEW_ROW_1, HYPER[2]])
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
    row0, rows_dev, state = a.hyper[0].clone(), a.hyper_dev.clone(), [getattr(a, n).clone() for n in STATE]
    a.set_hyper(1, **NEW_ROW_1)
    assert torch.equal(a.hyper, b.hyper) and torch.equal(a.hyper_dev.cpu(), b.hyper) and torch.equal(a.hyper[0], row0)
    assert torch.equal(a.hyper_dev[0], rows_dev[0]) and torch.equal(a.hyper_dev[2], rows_dev[2])
    assert a.learning_rates == b.learning_rates and a.learning_rates[1] == NEW_ROW_1["learning_rate"]
    for n, x in zip(STATE, state):                   # (no optimiser was named: the state is what it was)
        assert torch.equal(getattr(a, n), x), n
    for pp in (a, b):
        _iteration(pp)
    torch.cuda.synchronize()
    for name in BUFS + ("last_val", "stats") + STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.upd_t.tolist() == [2] * P


def test_set_hyper_with_another_optimizer_starts_the_members_state_afresh():
    pp = _population()
    pp.learn(1, T)
    before = {n: getattr(pp, n).clone() for n in STATE}
    assert all(bool((before[n][p] != 0).any()) for n in ("upd_s0", "upd_t") for p in range(P))
    assert bool((before["upd_s1"][1] != 0).any())                 # (member 1 is Adam's)
    keep, keep_dev = pp.hyper.clone(), pp.hyper_dev.clone()
    for kw, word in ((dict(gamma=1.5), "gamma"), (dict(vf_coef=0.1, learning_rate=0.0), "learning_rate"),
                     (dict(n_steps=8), "n_steps"), (dict(clip_range=0.2), "clip_range"),
                     (dict(optimizer="sgd"), "optimizer"), (dict(ent_coef=float("nan")), "ent_coef")):
        with pytest.raises(ValueError, match=word):
            pp.set_hyper(1, **kw)
    with pytest.raises(ValueError, match="member 3"):
        pp.set_hyper(3, gamma=0.5)
    assert torch.equal(pp.hyper, keep) and torch.equal(pp.hyper_dev, keep_dev)
    pp.set_hyper(2, optimizer="rmsprop")                          # (its own: nothing starts afresh)
    pp.set_hyper(1, optimizer="rmsprop_tf", max_grad_norm=0.3)
    torch.cuda.synchronize()
    assert pp.optimizers == ["rmsprop_tf", "rmsprop_tf", "rmsprop"] and float(pp.hyper_dev[1, 7]) == 2.0
    assert float(pp.hyper_dev[1, 4]) == 0.3
    assert bool((pp.upd_s0[1] == 1).all()) and bool((pp.upd_s1[1] == 0).all()) and int(pp.upd_t[1]) == 0
    assert torch.equal(pp.flat, before["flat"])
    for n in ("upd_s0", "upd_s1", "upd_t"):
        assert torch.equal(getattr(pp, n)[0], before[n][0]) and torch.equal(getattr(pp, n)[2], before[n][2]), n
    pp.set_hyper(1, optimizer="adam")
    torch.cuda.synchronize()
    assert bool((pp.upd_s0[1] == 0).all()) and bool((pp.upd_s1[1] == 0).all()) and int(pp.upd_t[1]) == 0
    _iteration(pp)
    torch.cuda.synchronize()
    assert pp.upd_t.tolist() == [2, 1, 2] and bool(torch.isfinite(pp.flat[:, :pp.n_params]).all())


def test_copy_member_makes_the_target_the_source_and_leaves_the_others_alone():
    pp = _population()
    pp.learn(1, T)
    before = {name: getattr(pp, name).clone() for name in STATE + ("hyper", "hyper_dev")}
    assert not torch.equal(pp.flat[0], pp.flat[2]) and not torch.equal(pp.upd_s0[0], pp.upd_s0[2])
    pp.copy_member(1, 2, hyper=False)
    torch.cuda.synchronize()
    for name in STATE:
        x = getattr(pp, name)
        assert torch.equal(x[2], before[name][1]) and torch.equal(x[:2], before[name][:2]), name
    assert torch.equal(pp.hyper, before["hyper"]) and torch.equal(pp.hyper_dev, before["hyper_dev"])
    pp.copy_member(1, 1)                                  # (onto itself: nothing)
    pp.flat[2].fill_(0.0)
    pp.copy_member(0, 2)
    torch.cuda.synchronize()
    for name in STATE + ("hyper", "hyper_dev"):
        x = getattr(pp, name)
        assert torch.equal(x[2], before[name][0]) and torch.equal(x[:2], before[name][:2]), name
    assert pp.learning_rates == [HYPER[0]["learning_rate"], HYPER[1]["learning_rate"], HYPER[0]["learning_rate"]]
    assert pp.optimizers == ["rmsprop_tf", "adam", "rmsprop_tf"]
    with pytest.raises(ValueError, match="member 3"):
        pp.copy_member(0, 3)
    # the twins stay twins only as far as their envs and reward constants let them: they train on
    _iteration(pp)
    torch.cuda.synchronize()
    assert pp.upd_t.tolist() == [2] * P and bool(torch.isfinite(pp.flat[:, :pp.n_params]).all())


def test_control_test_flies_before_every_iteration_with_and_without_a_graph():
    from b747_rl_ctrl_amd import ControlTest
    plain, _ = _plain_run()
    runs = []
    for use_graph in (False, True):
        pop = _population()
        ct = pop.control_test = ControlTest(pop, REFS, log_interval=T, window_length=3, tk=1.0)
        hist = pop.learn(2, T, use_graph=use_graph)
        torch.cuda.synchronize()
        assert ct.evaluations == 2 and ct.count.tolist() == [2] * P
        for h in hist:
            assert sorted(set(h) - set(LOG_KEYS)) == ["transfer_overshoot", "transfer_quality", "transfer_settling_time"]
            for k in ("transfer_overshoot", "transfer_quality", "transfer_settling_time"):
                assert tuple(h[k].shape) == (P,) and bool(torch.isfinite(h[k]).all()), k
        # the evaluations read the policies and write nothing of the learner's
        for name in BUFS + ("last_val", "stats") + STATE:
            assert torch.equal(getattr(pop, name), getattr(plain, name)), name
        runs.append((hist, ct))
    assert _same_history(runs[0][0], runs[1][0])
    for name in ("window_mean", "last", "best_quality", "best_eval", "best_flat"):
        assert torch.equal(getattr(runs[0][1], name), getattr(runs[1][1], name)), name


def test_the_arguments_are_checked():
    pp, _ = _plain_run()
    for kw in (dict(minibatch_order=lambda *a: None), dict(sample_order="device")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            pp.learn(1, T, **kw)
    with pytest.raises(ValueError, match="minibatch_order"):
        pp.train(T, minibatch_order=lambda *a: None)
    with pytest.raises(ValueError, match="sample_order"):
        _population(sample_order="device")
    from b747_rl_ctrl_amd import PopulationA2C
    with pytest.raises(ValueError, match="tile"):
        PopulationA2C(_env(N), 2, EPP, _cfg())                    # 2 x 64 envs do not cover 192
    with pytest.raises(ValueError, match="envs_per_member"):
        PopulationA2C(_env(N - 8), P, EPP, _cfg())                # a partial last member: no common batch
    with pytest.raises(ValueError, match="gamma"):
        _population([{"gamma": 2.0}, {}, {}])
    with pytest.raises(ValueError, match="optimizer"):
        PopulationA2C(_env(N), P, EPP, _cfg(optimizer="sgd"))
