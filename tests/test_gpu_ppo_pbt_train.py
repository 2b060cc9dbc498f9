"""PopulationPPO.exploit / PopulationA2C.exploit and ppo.PBT in training (b747_ppo_exploit).

Shape: that of tests/test_gpu_ppo_control_test.py shrunk (P = 4 members of 64 envs, T = 8, batch 128, two epochs,
FAITHFUL, train tk 0.3); the test env flies tk 1.0 against +-5 degrees; log_interval 8, so every iteration evaluates
once.  fraction 0.5: two losers, each drawing one of two winners.

  (a) exploit() against a twin population driven from the host: the twin reads the score, calls the NumPy reference
      (tests/exploit_ref.py), then copy_member and set_hyper per replaced member and gathers its tracker's window books
      by hand.  Parameters, Adam rows, step counts, the device table and the books are torch.equal, and so are the
      next iteration's parameters and history.
  (b) learn(use_graph=True) with PBT(interval=2) over five iterations (exploits before iterations 2 and 4) gives the
      bits of use_graph=False: parameters, state, history, pbt_source included -- and pbt_source is the reference's plan
  (c) the same for PopulationA2C with mixed optimisers: the optimiser column and both state rows travel together, and
      `optimizers` is right after sync_hyper
  (d) score="mean_reward" without a control test
  (e) rewards=True moves the rew rows, and the next rollout's rewards are the source configuration's
  (f) a run with pbt = None keeps today's history keys

Every comparison first asserts, on the REFERENCE's src_of, that the plan replaces somebody: otherwise it would show
nothing."""
import math

import numpy as np
import pytest
import torch

import exploit_ref as R

pytestmark = pytest.mark.gpu

P, EPP, T, BATCH, EPOCHS = 4, 64, 8, 128, 2
N = P * EPP
SEED, ENV_SEED, SEEDS = (1 << 33) + 1, 3, [5, 6, 7, 8]
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3},
               {"k0": 2.0, "kf": 0.1, "k1": 2}]
HYPER = [dict(learning_rate=3e-4, ent_coef=0.005, clip_range=0.2, gamma=0.99),
         dict(learning_rate=9.5e-4, ent_coef=0.0095, clip_range=0.1, gamma=0.9, vf_coef=0.25),
         dict(learning_rate=1.1e-5, ent_coef=0.0, clip_range=0.3, gae_lambda=0.8, max_grad_norm=5.0),
         dict(learning_rate=5e-4, ent_coef=0.002, clip_range=0.25, gamma=0.95)]
A2C_HYPER = [dict(learning_rate=7e-4, ent_coef=0.01, optimizer="rmsprop_tf"),
             dict(learning_rate=1e-3, ent_coef=0.0, vf_coef=0.25, gamma=0.9, optimizer="adam"),
             dict(learning_rate=3e-4, ent_coef=0.005, max_grad_norm=10.0, gae_lambda=0.95, optimizer="rmsprop"),
             dict(learning_rate=5e-4, ent_coef=0.09, gamma=0.95, optimizer="adam")]
REFS = [math.radians(v) for v in (5.0, -5.0)]
STATE = ("flat", "upd_m", "upd_v", "upd_t", "step_base", "hyper_dev")
A2C_STATE = ("flat", "upd_s0", "upd_s1", "upd_t", "step_base", "hyper_dev")
BOOKS = ("ring", "count", "last", "window_mean", "best_quality", "best_eval", "best_flat")
PPO_KEYS = {"entropy_loss", "policy_gradient_loss", "value_loss", "approx_kl", "clip_fraction", "loss",
            "explained_variance", "std", "pg_term_scale", "kl_term_scale", "policy_loss", "mean_reward"}


def _env():
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    return BatchControllerEnv(N, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, sample_time=0.05,
                              seed=ENV_SEED, variant="faithful")


def _ppo(hyper=HYPER, rew_configs=REW_CONFIGS, control_test=True):
    from b747_rl_ctrl_amd import ControlTest
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS, ent_coef=0.01)
    pop = PopulationPPO(_env(), P, EPP, cfg, seeds=SEEDS, rew_configs=rew_configs, seed=SEED, batched_update=True,
                        sample_order="device", hyper=hyper)
    if control_test:
        pop.control_test = ControlTest(pop, REFS, log_interval=T, window_length=3, tk=1.0)
    return pop


def _a2c():
    from b747_rl_ctrl_amd import ControlTest, PopulationA2C
    from b747_rl_ctrl_amd.ppo import A2CConfig
    cfg = A2CConfig.reference(n_steps=T, normalize_advantage=True, rms_eps=1e-7)
    pop = PopulationA2C(_env(), P, EPP, cfg, seeds=SEEDS, rew_configs=REW_CONFIGS, seed=SEED, hyper=A2C_HYPER)
    pop.control_test = ControlTest(pop, REFS, log_interval=T, window_length=3, tk=1.0)
    return pop


def _eq(a, b):
    """torch.equal with NaN positions equal"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


def _same_history(a, b):
    return len(a) == len(b) and all(sorted(x) == sorted(y) and all(_eq(x[k], y[k]) for k in x) for x, y in zip(a, b))


def _same_state(a, b, names):
    return all(_eq(getattr(a, k), getattr(b, k)) for k in names) and \
        all(_eq(getattr(a.control_test, k), getattr(b.control_test, k)) for k in BOOKS)


def _rule(pop, explore):
    """The explore rows exploit() passes for `explore` (None: the class's default)"""
    from b747_rl_ctrl_amd import ppo
    rule = pop.PBT_EXPLORE if explore is None else explore
    return ppo.explore_table(pop._HYPER_KEYS, pop._check_value, rule, "test") if rule else None


def _record(pop):
    """Make pop.exploit keep what the reference needs to restate each call: the score, step_base, the round and the
    table before it"""
    calls, exploit = [], pop.exploit

    def wrapped(score=None, fraction=0.25, explore=None, rewards=False, round=None):
        s = pop.control_test.objective() if score is None else score
        calls.append(dict(score=s.cpu().numpy().copy(), sb=int(pop.step_base.item()), round=pop._exploits,
                          table=None if pop.hyper is None else pop.hyper_dev.cpu().numpy().copy(),
                          n_replace=int(P * fraction), rows=_rule(pop, explore) if pop.hyper is not None else None))
        return exploit(score, fraction, explore, rewards, round)
    pop.exploit = wrapped
    return calls


def _reference_plans(calls):
    """The reference's (src_of, rows) of every recorded call; each must replace somebody"""
    out = []
    for c in calls:
        src, rows = R.plan(c["score"], c["n_replace"], SEED, c["sb"], c["round"], c["table"], c["rows"])
        assert (src != np.arange(P)).any(), f"the reference plan replaces nobody (scores {c['score']})"
        out.append((src, rows))
    return out


def _same_bits(dev, ref):
    return np.array_equal(dev.cpu().numpy().view(np.int64), np.ascontiguousarray(ref).view(np.int64))


# ------------------------------------------------------------------------------------------------------------ (a) --
def test_exploit_is_the_host_loop_of_copy_member_and_set_hyper_on_a_twin():
    from b747_rl_ctrl_amd.ppo import HYPER_COLUMN
    pop, twin = _ppo(), _ppo()
    h1, h2 = pop.learn(2), twin.learn(2)
    assert _same_history(h1, h2) and _same_state(pop, twin, STATE)
    assert "pbt_source" not in h1[0]

    # the twin's step, decided by the reference from a host read of the score
    score = twin.control_test.objective().cpu().numpy()
    src, rows = R.plan(score, 2, SEED, int(twin.step_base.item()), 0, twin.hyper.numpy(), _rule(twin, None))
    replaced = [p for p in range(P) if src[p] != p]
    assert replaced, f"the reference plan replaces nobody (scores {score})"
    assert not np.array_equal(rows[replaced], twin.hyper.numpy()[src[replaced]])       # the exploration shows
    for p in replaced:
        twin.copy_member(int(src[p]), p)
        twin.set_hyper(p, **{k: float(rows[p, c]) for k, c in HYPER_COLUMN.items()})
    ct = twin.control_test
    idx = torch.from_numpy(src.astype(np.int64)).cuda()
    ct.ring.copy_(ct.ring[:, idx])
    for x in (ct.count, ct.last, ct.window_mean):
        x.copy_(x[idx])

    got = pop.exploit(fraction=0.5)
    assert got is pop.src_of and got.dtype == torch.int32 and got.cpu().tolist() == src.tolist()
    assert _same_bits(pop.hyper_dev, rows) and _same_bits(twin.hyper_dev, rows)
    assert _same_state(pop, twin, STATE)
    assert not torch.equal(pop.hyper, twin.hyper)               # the mirror is stale until it is asked for
    pop.sync_hyper()
    assert torch.equal(pop.hyper, twin.hyper) and pop.learning_rates == twin.learning_rates
    assert list(pop._lr) == list(twin._lr)

    # what follows is the same training
    h1, h2 = pop.learn(2), twin.learn(2)
    assert _same_history(h1, h2) and _same_state(pop, twin, STATE)
    # a second step takes round 1, and set_hyper after it reads a fresh mirror
    score = pop.control_test.objective().cpu().numpy()
    src2, rows2 = R.plan(score, 2, SEED, int(pop.step_base.item()), 1, pop.hyper_dev.cpu().numpy(), _rule(pop, {}))
    assert (src2 != np.arange(P)).any()
    assert pop.exploit(fraction=0.5, explore={}).cpu().tolist() == src2.tolist() and _same_bits(pop.hyper_dev, rows2)
    pop.set_hyper(0, vf_coef=0.125)
    rows2[0, HYPER_COLUMN["vf_coef"]] = 0.125
    assert _same_bits(pop.hyper_dev, rows2) and _same_bits(pop.hyper, rows2)


# ------------------------------------------------------------------------------------------------------------ (b) --
def _pbt_run(make, state, use_graph, iterations=5, **pbt_kw):
    from b747_rl_ctrl_amd import PBT
    pop = make()
    pop.pbt = PBT(2, fraction=0.5, **pbt_kw)
    calls = _record(pop)
    hist = pop.learn(iterations, use_graph=use_graph)
    return pop, hist, calls


@pytest.mark.parametrize("make,state", [(_ppo, STATE), (_a2c, A2C_STATE)], ids=["ppo", "a2c"])
def test_learn_with_a_pbt_replays_as_a_graph_with_the_same_bits_and_the_references_plans(make, state):
    a, ha, calls = _pbt_run(make, state, False)
    plans = _reference_plans(calls)
    assert len(plans) == 2 and [c["round"] for c in calls] == [0, 1]
    me = np.arange(P)
    for it, entry in enumerate(ha):
        want = plans[it // 2 - 1][0] if it in (2, 4) else me
        assert entry["pbt_source"].dtype == torch.int32 and entry["pbt_source"].cpu().tolist() == want.tolist(), it
    # the table after the last step is the reference's (no update writes it)
    assert _same_bits(a.hyper_dev, plans[-1][1])
    b, hb, _ = _pbt_run(make, state, True)
    assert _same_history(ha, hb) and _same_state(a, b, state)
    # and it is not the run without a schedule
    plain = make()
    hp = plain.learn(5)
    assert "pbt_source" not in hp[0] and _same_history([{k: v for k, v in ha[1].items() if k != "pbt_source"}], [hp[1]])
    assert not _eq(a.flat, plain.flat)


# ------------------------------------------------------------------------------------------------------------ (c) --
def test_a2c_members_take_the_optimiser_column_and_both_state_rows_together():
    from b747_rl_ctrl_amd.ppo import A2C_HYPER_COLUMN
    pop = _a2c()
    pop.learn(2)
    names = pop.optimizers
    assert names == [h["optimizer"] for h in A2C_HYPER]
    before = {k: getattr(pop, k).clone() for k in A2C_STATE}
    score = pop.control_test.objective().cpu().numpy()
    src, rows = R.plan(score, 2, SEED, int(pop.step_base.item()), 0, before["hyper_dev"].cpu().numpy(), _rule(pop, None))
    moved = src != np.arange(P)
    assert moved.any() and any(names[src[p]] != names[p] for p in range(P)), (score, src)
    assert pop.exploit(fraction=0.5).cpu().tolist() == src.tolist()
    idx = torch.from_numpy(src.astype(np.int64)).cuda()
    for k in ("flat", "upd_s0", "upd_s1", "upd_t"):
        assert torch.equal(getattr(pop, k).view(torch.int32 if k != "upd_t" else torch.int64),
                           before[k][idx].view(torch.int32 if k != "upd_t" else torch.int64)), k
    assert _same_bits(pop.hyper_dev, rows)
    col = A2C_HYPER_COLUMN["optimizer"]
    assert torch.equal(pop.hyper_dev[:, col], before["hyper_dev"][idx, col])
    assert pop.optimizers == [names[q] for q in src]                 # (sync_hyper first: the mirror was stale)
    assert _same_bits(pop.hyper, rows)
    pop.learn(1)                                                      # the moved state rows serve the moved optimiser
    assert bool(torch.isfinite(pop.flat[:, :pop.n_params]).all())


# ------------------------------------------------------------------------------------------------------------ (d) --
def test_mean_reward_ranks_without_a_control_test():
    from b747_rl_ctrl_amd import PBT
    pop = _ppo(control_test=False)
    pop.pbt = PBT(1, fraction=0.5, score="mean_reward", explore={"clip_range": (0.5, 2.0, 0.05, 0.4)})
    calls = _record(pop)
    hist = pop.learn(3)
    plans = _reference_plans(calls)
    assert len(plans) == 2
    for c, entry in zip(calls, hist):            # the score of step k is iteration k - 1's mean reward, as float64
        assert np.array_equal(c["score"], entry["mean_reward"].double().cpu().numpy())
    assert hist[0]["pbt_source"].cpu().tolist() == list(range(P))
    assert [h["pbt_source"].cpu().tolist() for h in hist[1:]] == [s.tolist() for s, _ in plans]
    assert _same_bits(pop.hyper_dev, plans[-1][1])
    assert "transfer_quality" not in hist[0]


# ------------------------------------------------------------------------------------------------------------ (e) --
def test_rewards_true_moves_the_reward_rows_and_the_next_rollout_uses_them():
    score = np.array([0.5, 0.125, 0.75, 0.25])
    src, _ = R.plan(score, 2, SEED, 0, 0)
    replaced = [p for p in range(P) if src[p] != p]
    assert replaced and any(REW_CONFIGS[src[p]] != REW_CONFIGS[p] for p in replaced)
    dev_score = torch.from_numpy(score).cuda()
    pop, own = _ppo(hyper=None, control_test=False), _ppo(hyper=None, control_test=False)
    twin = _ppo(hyper=None, control_test=False, rew_configs=[REW_CONFIGS[q] for q in src])
    for x in (pop, own, twin):
        x.env.reset()
    rew = pop.rew.clone()
    assert pop.exploit(dev_score, fraction=0.5, rewards=True).cpu().tolist() == src.tolist()
    assert own.exploit(dev_score, fraction=0.5).cpu().tolist() == src.tolist()
    for x in (twin.flat, twin.upd_m, twin.upd_v, twin.upd_t):          # (no table: copy_member needs one)
        for p in replaced:
            x[p].copy_(x[int(src[p])])
    assert torch.equal(pop.rew, rew[torch.from_numpy(src.astype(np.int64)).cuda()]) and torch.equal(pop.rew, twin.rew)
    assert torch.equal(own.rew, rew) and torch.equal(pop.flat, twin.flat) and torch.equal(pop.flat, own.flat)
    for x in (pop, own, twin):
        x.collect_rollouts()
    assert torch.equal(pop.rew_buf, twin.rew_buf) and torch.equal(pop.act_buf, twin.act_buf)
    assert torch.equal(pop.act_buf[0], own.act_buf[0]) and not torch.equal(pop.rew_buf, own.rew_buf)
    cols = pop.rew_buf.reshape(T, P, EPP) != own.rew_buf.reshape(T, P, EPP)
    assert [p for p in range(P) if bool(cols[:, p].any())] == [p for p in replaced if REW_CONFIGS[src[p]] != REW_CONFIGS[p]]


# ------------------------------------------------------------------------------------------------------------ (f) --
def test_without_a_pbt_the_history_keys_are_todays():
    pop = _ppo()
    assert pop.pbt is None
    hist = pop.learn(2)
    transfer = {"transfer_settling_time", "transfer_overshoot", "transfer_quality"}
    assert all(set(h) == PPO_KEYS | transfer for h in hist)
    assert pop._exploits == 0 and pop.src_of.cpu().tolist() == list(range(P)) and not pop._hyper_stale
