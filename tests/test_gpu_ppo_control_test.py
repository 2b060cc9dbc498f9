"""ppo.ControlTest in training (learn(control_test=...) of PPO, the control_test attribute of PopulationPPO;
b747_ppo_track_best): the reference's ControlTestCallback kept on the device.

Shape: that of tests/test_gpu_ppo_population_device_order_train.py (P = 3 members of 64 envs, T = 8, batch 128, two
epochs, FAITHFUL, train tk 0.3), four iterations; the test env flies tk 1.0 against +-5 and +-10 degrees; log_interval 5
(pushes 1, 2, 1, 2) and a window of 3.

  (a) against a twin population driven by a host loop that calls the existing step_tests (a fresh env every time) before
      each iteration and feeds the NumPy reference (tests/control_test_ref.py): the per-env metrics the tracker read
      equal step_tests' with torch.equal, everything downstream of the kernel's own `last` is exact, and best_flat[p] is
      the twin's flat[p] of the iteration of best_eval[p]
  (b) training is not disturbed: parameters, Adam state, step_base and the rollout buffers are those of a run without
  (c) learn(use_graph=True) gives the bits of use_graph=False, history entries and ControlTest state
  (d) a single PPO(fused=True, fused_update=True) against PPO.step_tests, the same way (P = 1)
  (e) one recorded run of tests/golden/tb_transfer_first_log.json with its reconstructed weights and main.py's test
      env (tk 20), one evaluation: window_mean against the recorded transfer_custom/* at the tolerance
      tests/test_gpu_tb_pin.py holds the step tests to"""
import math

import numpy as np
import pytest
import torch

import control_test_ref as R

pytestmark = pytest.mark.gpu

P, EPP, T, BATCH, EPOCHS, ITERS = 3, 64, 8, 128, 2, 4
N = P * EPP
SEED, ENV_SEED, SEEDS = (1 << 33) + 1, 3, [5, 6, 7]
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3}]
REFS = [math.radians(v) for v in (5.0, -5.0, 10.0, -10.0)]
TEST_TK, LOG_INTERVAL, WINDOW = 1.0, 5, 3
PUSHES = [1, 2, 1, 2]
BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "last_val")
STATE = ("flat", "upd_m", "upd_v", "upd_t", "step_base")
CT_STATE = ("eval_out", "ring", "count", "last", "window_mean", "best_quality", "best_eval", "best_flat")


def _env(n=N):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, sample_time=0.05,
                              seed=ENV_SEED, variant="faithful")


def _population():
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS, ent_coef=0.01)
    return PopulationPPO(_env(), P, EPP, cfg, seeds=SEEDS, rew_configs=REW_CONFIGS, seed=SEED, batched_update=True,
                         sample_order="device")


def _control_test(learner):
    from b747_rl_ctrl_amd import ControlTest
    return ControlTest(learner, REFS, log_interval=LOG_INTERVAL, window_length=WINDOW, tk=TEST_TK)


def _eq(a, b):
    """torch.equal with NaN positions equal"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


def _snapshots(ct):
    """Make ct.evaluate keep a copy of the tracker's state after every call"""
    snaps, evaluate = [], ct.evaluate

    def wrapped(repeat=1):
        evaluate(repeat)
        snaps.append({k: getattr(ct, k).clone() for k in CT_STATE} | {"repeat": repeat})
    ct.evaluate = wrapped
    return snaps


def _check_books(snaps, twin_outs, twin_flats, n_members, tk):
    """(a): the evaluations `snaps` of a ControlTest against the step_tests results and parameter copies of its twin"""
    from b747_rl_ctrl_amd.evaluate import quality
    idx = (torch.arange(n_members)[:, None] * 64 + torch.arange(len(REFS))[None]).cuda()
    repeats = [s["repeat"] for s in snaps]
    for it, (s, out) in enumerate(zip(snaps, twin_outs)):
        ev, vref = s["eval_out"], out["env"].ref[0].to(torch.float64)
        rows = {k: ev[j][idx] for j, k in enumerate(("overshoot", "rise_time", "settling_time", "static_error", "itse",
                                                     "length", "return"))}
        want = {k: out[k].reshape(n_members, -1) for k in ("settling_time", "overshoot", "quality", "rise_time",
                                                           "static_error", "return")}
        assert _eq(rows["settling_time"], want["settling_time"]), it
        assert _eq(rows["overshoot"].abs(), want["overshoot"]), it
        assert _eq(quality(rows["itse"], vref[idx], tk), want["quality"]), it       # (the ITSE, through step_tests' own exp)
        for k in ("rise_time", "static_error", "return"):
            assert _eq(rows[k], want[k]), (it, k)
        # last: NumPy's means of those values; the quality column within 4 ulp (the device's exp against NumPy's)
        means = R.means([rows["settling_time"].tolist(), rows["overshoot"].abs().tolist(),
                         R.quality(rows["itse"].cpu().numpy(), vref[idx].cpu().numpy(), tk).tolist()])
        last = s["last"].cpu().numpy()
        assert R.same(last[:, :2], means[:, :2]), (it, last, means)
        ulps = np.abs(last[:, 2] - means[:, 2]) / np.spacing(means[:, 2])
        dev_q = np.array([np.mean(r) for r in want["quality"].tolist()])
        print(f"evaluation {it}: quality {last[:, 2]}: {ulps} ulp from NumPy, "
              f"{'bit-equal to' if R.same(last[:, 2], dev_q) else 'not bit-equal to'} evaluate.quality's mean on the device")
        assert np.all(ulps <= 4), (it, last, means)
    ref = R.track([s["last"].cpu().numpy() for s in snaps], repeats, WINDOW)
    for it, (s, want) in enumerate(zip(snaps, ref)):
        print(f"evaluation {it}: margins {want['margin']}, saved {want['saved']}")
        for k in ("window_mean", "best_quality", "best_eval", "count"):
            assert R.same(s[k].cpu().numpy(), want[k]), (it, k, s[k], want[k])
        first_push = sum(repeats[:it])
        for p in range(n_members):
            be = int(want["best_eval"][p])
            saved_it = 0 if be < 0 else max(i for i in range(len(repeats)) if sum(repeats[:i]) <= be)
            assert be < first_push + repeats[it]
            assert torch.equal(s["best_flat"][p], twin_flats[saved_it].reshape(n_members, -1)[p]), (it, p, be, saved_it)
    assert R.same(snaps[-1]["ring"].cpu().numpy(), R.ring([s["last"].cpu().numpy() for s in snaps], repeats, WINDOW))
    assert any(w["saved"].any() for w in ref), "nothing was ever saved: the scenario checks no snapshot"


@pytest.fixture(scope="module")
def direct():
    """learn(4) with a control test, calls made directly; the tracker's state after every evaluation"""
    pop = _population()
    ct = pop.control_test = _control_test(pop)
    snaps = _snapshots(ct)
    hist = pop.learn(ITERS, T)
    torch.cuda.synchronize()
    return {"pop": pop, "ct": ct, "snaps": snaps, "hist": hist}


def test_a_the_books_are_the_callbacks_on_a_twin_populations_step_tests(direct):
    twin, outs, flats = _population(), [], []
    twin.env.reset()
    for it in range(ITERS):
        outs.append(twin.step_tests(REFS, tk=TEST_TK))
        flats.append(twin.flat.clone())
        twin.collect_rollouts(T)
        twin.compute_gae(T)
        twin.train(T)
    torch.cuda.synchronize()
    snaps, ct = direct["snaps"], direct["ct"]
    assert [s["repeat"] for s in snaps] == PUSHES and ct.evaluations == ITERS
    assert ct.env.n == (P - 1) * 64 + len(REFS) and ct.steps == 20
    _check_books(snaps, outs, flats, P, TEST_TK)
    for name in STATE + BUFS:
        assert torch.equal(getattr(direct["pop"], name), getattr(twin, name)), name
    # the accessors
    assert torch.equal(ct.objective(), ct.window_mean[:, 2]) and int(ct.best_member()) == int(ct.best_quality.argmax())
    p = int(ct.best_member())
    net = ct.best(p)
    assert torch.equal(net.flat_params(), ct.best_flat[p, :direct["pop"].n_params])
    # the history entries are the windowed means after each iteration's pushes
    for it, h in enumerate(direct["hist"]):
        for j, k in enumerate(("transfer_settling_time", "transfer_overshoot", "transfer_quality")):
            assert tuple(h[k].shape) == (P,) and _eq(h[k], snaps[it]["window_mean"][:, j]), (it, k)


def test_b_training_is_not_disturbed(direct):
    plain = _population()
    hist = plain.learn(ITERS, T)
    torch.cuda.synchronize()
    for name in STATE + BUFS + ("perm", "stats"):
        assert torch.equal(getattr(direct["pop"], name), getattr(plain, name)), name
    for x, y in zip(direct["hist"], hist):
        assert sorted(set(x) - set(y)) == ["transfer_overshoot", "transfer_quality", "transfer_settling_time"]
        for k in y:
            assert torch.equal(x[k], y[k]), k
    assert plain.control_test is None


def test_c_graph_iterations_are_the_direct_calls(direct):
    graph = _population()
    ct = graph.control_test = _control_test(graph)
    hist = graph.learn(ITERS, T, use_graph=True)
    torch.cuda.synchronize()
    assert graph._graph is not None and direct["pop"]._graph is None
    for name in STATE + BUFS + ("perm", "stats"):
        assert torch.equal(getattr(graph, name), getattr(direct["pop"], name)), name
    for name in CT_STATE:
        assert _eq(getattr(ct, name), getattr(direct["ct"], name)), name
    assert len(hist) == len(direct["hist"])
    for it, (x, y) in enumerate(zip(hist, direct["hist"])):
        assert sorted(x) == sorted(y)
        for k in x:
            assert _eq(x[k], y[k]), (it, k)


def test_no_pushes_launch_nothing_and_the_entries_stay_nan():
    from b747_rl_ctrl_amd import ControlTest
    pop = _population()
    ct = pop.control_test = ControlTest(pop, REFS, log_interval=3 * T + 1, window_length=WINDOW, tk=TEST_TK)
    hist = pop.learn(3, T)          # 24 callback calls: none is a multiple of 25
    torch.cuda.synchronize()
    assert ct.evaluations == 0 and ct.count.tolist() == [0] * P and ct.best_eval.tolist() == [-1] * P
    assert all(bool(torch.isnan(h[k]).all()) for h in hist for k in ("transfer_quality", "transfer_overshoot",
                                                                      "transfer_settling_time"))
    assert torch.equal(ct.best_flat[:, :pop.n_params], _population().flat[:, :pop.n_params])
    with pytest.raises(ValueError, match="repeat=257"):
        ct.evaluate(257)
    with pytest.raises(ValueError, match="another learner"):
        other = _population()
        other.control_test = ct
        other.learn(1, T)


def test_d_a_single_learner_against_its_own_step_tests():
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS, ent_coef=0.01)
    iters = 3
    ppo = PPO(_env(EPP), cfg, seed=11, fused=True, fused_update=True)
    ct = _control_test(ppo)
    snaps = _snapshots(ct)
    hist = ppo.learn(iters, T, control_test=ct)
    twin, outs, flats = PPO(_env(EPP), cfg, seed=11, fused=True, fused_update=True), [], []
    twin.last_obs.copy_(twin.env.reset())
    twin._last_obs_from_env = False
    for it in range(iters):
        outs.append(twin.step_tests(REFS, tk=TEST_TK))
        flats.append(twin.flat.clone())
        twin.collect_rollouts(T)
        twin.compute_gae(T)
        twin.train(T)
    torch.cuda.synchronize()
    assert [s["repeat"] for s in snaps] == PUSHES[:iters] and ct.env.n == len(REFS) and ct.n_members == 1
    _check_books(snaps, outs, flats, 1, TEST_TK)
    assert torch.equal(ppo.flat, twin.flat) and torch.equal(ppo.upd_m, twin.upd_m) and torch.equal(ppo.upd_t, twin.upd_t)
    for it, h in enumerate(hist):
        assert tuple(h["transfer_quality"].shape) == (1,)
        assert _eq(h["transfer_quality"], snaps[it]["window_mean"][:, 2])
    assert "transfer_quality" not in twin.learn(1, T)[0]


@pytest.mark.parametrize("variant", ["fast", "faithful"])
def test_e_a_recorded_runs_first_transfer_log(variant):
    import tb_transfer as TB
    from b747_rl_ctrl_amd import (BatchControllerEnv, ControlTest, CtrlMode, CtrlType, ObservationType, ResetRefMode,
                                  RewardType)
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    runs = TB.load_fixture()
    name = next(n for n in sorted(runs) if TB.split_run(n) == ("PID_LIKE", "DIRECT_CONTROL")
                and TB.reference_weights(n) is not None)
    mode, amax = TB.MODES["DIRECT_CONTROL"]
    env = BatchControllerEnv(64, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode(mode), reset_ref_mode=ResetRefMode.CONST, tk=TB.TK, sample_time=TB.SAMPLE_TIME,
                             action_max=amax, variant=variant)
    ppo = PPO(env, PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=1), fused=True)
    lin = [m for m in ppo.policy.pi_net if isinstance(m, torch.nn.Linear)] + [ppo.policy.action_net]
    with torch.no_grad():
        for layer, (w, b) in zip(lin, TB.reference_weights(name)):
            layer.weight.copy_(torch.as_tensor(w))
            layer.bias.copy_(torch.as_tensor(b))
    ppo.sync_params()
    ct = ControlTest(ppo, TB.REFS, state0=TB.STATE0.tolist(), log_interval=TB.CALLBACK_INTERVAL)
    assert ct.tk == TB.TK and ct.steps == 400 and ct.window_length == 30
    ct.evaluate()
    got, rec = ct.window_mean[0].tolist(), runs[name]
    print(f"{name} ({variant}): {got} against the record {[rec[k] for k in TB.KEYS]}")
    assert abs(got[0] - rec["settling_time"]) <= 0.0025 + 1e-6, (got, rec)
    err = TB.rel_err(got, rec)
    assert max(err[1:]) <= 1e-6, (got, rec, err)
    assert ct.count.tolist() == [1] and _eq(ct.last, ct.window_mean)
    assert ct.best_eval.tolist() == [0] and float(ct.best_quality) == got[2] and torch.equal(ct.best_flat[0], ppo.flat)
