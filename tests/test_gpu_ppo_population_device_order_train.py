"""Population training on device-drawn sample orders (ppo.PopulationPPO(sample_order="device"), b747_ppo_sample_orders;
DESIGN.md 18), and whole iterations replayed as one HIP graph (learn(use_graph=True)).

The device orders against the default path: a default population whose minibatch_order hook returns the reference's
local orders (tests/sample_orders_ref.py) for the step_base read after each rollout issues the same epoch calls on the
same perm, so parameters, Adam state and statistics are compared with torch.equal -- no tolerance.  The graph against
the same calls made directly, likewise.

Shape: P = 3 members of 64 envs, T = 8 steps (512 rows per member), batch_size 128 (four minibatches per member and
epoch), two epochs, two iterations, FAITHFUL.  tk 0.3 at sample_time 0.05: 6-step episodes, so the rollouts hold episode
ends and auto-resets."""
import pytest
import torch

import sample_orders_ref as R

pytestmark = pytest.mark.gpu

P, EPP, T, BATCH, EPOCHS = 3, 64, 8, 128, 2
N = P * EPP
SEED, ENV_SEED = (1 << 33) + 1, 3
SEEDS = [5, 6, 7]
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3}]
HYPER = [dict(learning_rate=3e-4, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, gamma=0.99,
              gae_lambda=0.95),
         dict(learning_rate=1e-3, clip_range=0.1, ent_coef=0.0, vf_coef=0.25, max_grad_norm=0.05, gamma=0.9,
              gae_lambda=0.6),
         dict(learning_rate=1e-4, clip_range=0.3, ent_coef=0.005, vf_coef=0.6, max_grad_norm=10.0, gamma=0.7,
              gae_lambda=1.0)]
NEW_ROW_1 = dict(learning_rate=5e-4, clip_range=0.15, gamma=0.95)
BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "last_val")
STATE = ("flat", "upd_m", "upd_v", "upd_t")


def _population(batched, hyper, sample_order, **kw):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    env = BatchControllerEnv(N, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                             CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, sample_time=0.05,
                             seed=ENV_SEED, variant="faithful")
    cfg = PPOConfig(n_steps=T, batch_size=BATCH, n_epochs=EPOCHS, ent_coef=0.01)
    return PopulationPPO(env, P, EPP, cfg, seeds=SEEDS, rew_configs=REW_CONFIGS, seed=SEED, batched_update=batched,
                         hyper=hyper, sample_order=sample_order, **kw)


def _same_state(a, b, what, names=BUFS + STATE):
    torch.cuda.synchronize()
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{what}: {name}"


def _same_hist(ha, hb, what):
    assert len(ha) == len(hb)
    for i, (x, y) in enumerate(zip(ha, hb)):
        assert sorted(x) == sorted(y)
        for k in x:
            assert tuple(x[k].shape) == (P,) and torch.equal(x[k], y[k]), f"{what}: iteration {i}: {k}"


@pytest.mark.parametrize("hyper", [None, HYPER], ids=["cfg", "hyper"])
@pytest.mark.parametrize("batched", [False, True], ids=["population", "batched"])
def test_device_orders_are_the_default_path_on_the_references_orders(batched, hyper):
    dev = _population(batched, hyper, "device")
    host = _population(batched, hyper, "host")
    seen = []

    def hook(epoch, T_, epp, p):
        sb = int(host.step_base)              # read after the rollout: what the order kernel reads on the device
        seen.append((sb, epoch, p))
        return torch.from_numpy(R.local_order(SEED, sb, epoch, p, T_ * epp).copy())     # (the cached array stays as it is)

    h_dev = dev.learn(2, T)
    h_host = host.learn(2, T, minibatch_order=hook)
    assert seen == [(sb, e, p) for sb in (T, 2 * T) for e in range(EPOCHS) for p in range(P)]
    _same_state(dev, host, "device orders against the hook")
    _same_hist(h_dev, h_host, "device orders against the hook")
    assert dev.upd_t.tolist() == [2 * EPOCHS * 4] * P and int(dev.step_base) == 2 * T
    # perm holds the last epoch's orders of the last iteration
    want = torch.from_numpy(R.reference_perm(P, T, EPP, N, SEED, 2 * T, EPOCHS - 1).copy())
    assert torch.equal(dev.perm.cpu(), want)
    assert bool(torch.isfinite(dev.flat[:, :dev.n_params]).all())


def test_device_orders_differ_from_the_default_streams_and_learn():
    dev = _population(True, None, "device")
    start = dev.flat.clone()
    dev.learn(1, T)
    host = _population(True, None, "host")
    host.learn(1, T)
    torch.cuda.synchronize()
    _same_state(dev, host, "the rollout does not depend on the orders", BUFS)
    assert not torch.equal(dev.flat, start) and not torch.equal(dev.flat, host.flat)


@pytest.mark.parametrize("hyper", [None, HYPER], ids=["cfg", "hyper"])
def test_graph_iterations_are_the_direct_calls(hyper):
    graph = _population(True, hyper, "device")
    direct = _population(True, hyper, "device")
    captured = None
    for it in range(2):
        hg = graph.learn(1, T, use_graph=True)
        hd = direct.learn(1, T)
        _same_state(graph, direct, f"iteration {it}")
        _same_hist(hg, hd, f"iteration {it}")
        assert torch.equal(graph.perm, direct.perm) and torch.equal(graph.stats, direct.stats)
        assert graph._graph is not None and direct._graph is None
        captured = captured or graph._graph
        assert graph._graph is captured, "the second iteration re-captured"
    assert int(graph.step_base) == 2 * T and graph.upd_t.tolist() == [2 * EPOCHS * 4] * P
    # ... and two iterations of one learn call
    hg, hd = graph.learn(2, T, use_graph=True), direct.learn(2, T)
    _same_state(graph, direct, "learn(2)")
    _same_hist(hg, hd, "learn(2)")
    assert graph._graph is captured


def test_set_hyper_and_copy_member_between_replays_need_no_new_capture():
    graph = _population(True, HYPER, "device")
    direct = _population(True, HYPER, "device")
    _same_hist(graph.learn(1, T, use_graph=True), direct.learn(1, T), "iteration 0")
    _same_state(graph, direct, "iteration 0")
    captured = graph._graph
    for pp in (graph, direct):
        pp.set_hyper(1, **NEW_ROW_1)
        pp.copy_member(0, 2)
    before = direct.flat.clone()
    _same_hist(graph.learn(1, T, use_graph=True), direct.learn(1, T), "iteration 1")
    _same_state(graph, direct, "iteration 1")
    assert graph._graph is captured, "set_hyper / copy_member caused a new capture"
    assert torch.equal(graph.hyper_dev.cpu(), graph.hyper) and torch.equal(graph.hyper, direct.hyper)
    assert graph.hyper[1, 0] == NEW_ROW_1["learning_rate"] and torch.equal(graph.hyper[2], graph.hyper[0])
    assert not torch.equal(direct.flat, before)
    # the new values were read: a population that never got them ends elsewhere
    other = _population(True, HYPER, "device")
    other.learn(1, T, use_graph=True)
    other.learn(1, T, use_graph=True)
    torch.cuda.synchronize()
    assert not torch.equal(other.flat[1], graph.flat[1]) and not torch.equal(other.flat[2], graph.flat[2])


def test_a_change_of_the_step_count_captures_again():
    graph = _population(True, None, "device")
    direct = _population(True, None, "device")
    graph.learn(1, T, use_graph=True)
    direct.learn(1, T)
    first = graph._graph
    _same_hist(graph.learn(1, T - 3, use_graph=True), direct.learn(1, T - 3), "T - 3")       # 320 rows: a partial minibatch
    _same_state(graph, direct, "T - 3", STATE)
    assert graph._graph is not first


def test_the_refusals():
    with pytest.raises(ValueError, match="sample_order=\"device\""):
        _population(True, None, "host").learn(1, T, use_graph=True)
    with pytest.raises(ValueError, match="batched_update=True"):
        _population(False, None, "device").learn(1, T, use_graph=True)
    with pytest.raises(ValueError, match="batched_update=True"):
        _population(False, HYPER, "device").learn(1, T, use_graph=True)
    order = lambda epoch, T_, epp, p: torch.randperm(T_ * epp)
    dev = _population(True, None, "device")
    with pytest.raises(ValueError, match="minibatch_order"):
        dev.learn(1, T, minibatch_order=order)
    with pytest.raises(ValueError, match="minibatch_order"):
        dev.learn(1, T, minibatch_order=order, use_graph=True)
    dev.env.reset()
    dev.collect_rollouts(T)
    dev.compute_gae(T)
    with pytest.raises(ValueError, match="minibatch_order"):
        dev.train(T, order)
    with pytest.raises(ValueError, match="sample_order='cuda'"):
        _population(True, None, "cuda")
