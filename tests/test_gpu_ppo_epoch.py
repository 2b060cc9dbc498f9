"""b747_ppo_epoch (include/b747.h ABI 13; PPO(fused_update=True, epoch_call=True)): every minibatch of one epoch from
one host call.

The yardstick is the two-call path it replaces -- a Python loop of b747_ppo_grad + b747_ppo_adam over the slices of
the same permutation, on copies of the same buffers.  The epoch call issues the same launches with the same arguments
in the same order, so everything it writes must be torch.equal to the loop's -- no tolerance.  (The two calls
themselves are held to fp64 torch by tests/test_gpu_ppo_update.py.)  The rollout of the first tests is synthetic: the
1,024-row set of tests/test_gpu_ppo_update.py, restated here from the same seeded CPU generator."""
import functools
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS, CLIP, ENT_COEF, VF_COEF = 1024, 0.2, 0.01, 0.5
MAX_NORM, LR, BETA1, BETA2, EPS = 0.5, 3e-4, 0.9, 0.999, 1e-5
SEED = 11
N_EPOCHS = 2


@functools.lru_cache(maxsize=None)
def _data(od):
    """theta (the flat parameters), the rollout buffers (obs, act, old_logp, adv, ret) and two permutations"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    g = torch.Generator().manual_seed(SEED + od)
    torch.manual_seed(SEED + od)
    policy = ActorCritic(od)
    with torch.no_grad():
        for p in policy.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
        policy.log_std.fill_(-0.3)
    old = ActorCritic(od)
    old.load_state_dict(policy.state_dict())
    with torch.no_grad():
        old.action_net.weight.add_(0.06 * torch.randn(old.action_net.weight.shape, generator=g))
        old.log_std.add_(0.05)
    obs = torch.randn(N_ROWS, od, generator=g)
    with torch.no_grad():
        mean_old, _ = old.double()(obs.double())
        act = (mean_old + old.log_std.exp() * torch.randn(N_ROWS, 1, generator=g, dtype=torch.float64)).float()
        old_logp = old.log_prob(mean_old, act.double()).float()
    adv = 0.3 + 1.5 * torch.randn(N_ROWS, generator=g)
    ret = torch.randn(N_ROWS, generator=g)
    perms = [torch.randperm(N_ROWS, generator=g) for _ in range(N_EPOCHS)]
    dev = torch.device("cuda")
    return (policy.flat_params().contiguous().to(dev), tuple(t.contiguous().to(dev) for t in (obs, act, old_logp, adv, ret)),
            tuple(p.to(dev) for p in perms))


class _State:
    """theta, Adam moments, step count, gradient, workspace and the statistics rows of one run"""

    def __init__(self, theta0, od, n_mb):
        from b747_rl_ctrl_amd import _lib
        dev = theta0.device
        self.theta = theta0.clone()
        self.m, self.v = torch.zeros_like(theta0), torch.zeros_like(theta0)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.grad = torch.full_like(theta0, float("nan"))
        self.ws = torch.empty(int(_lib.lib().b747_ppo_update_workspace(od)), dtype=torch.uint8, device=dev)
        self.stats = torch.full((N_EPOCHS * n_mb, 8), float("nan"), device=dev)

    def tensors(self):
        return {"theta": self.theta, "m": self.m, "v": self.v, "t": self.t, "grad": self.grad, "stats": self.stats}


def _loop_epoch(st, od, bufs, perm, batch_size, stats):
    """the parent path: per minibatch, b747_ppo_grad then b747_ppo_adam from the interpreter"""
    from b747_rl_ctrl_amd import _lib
    L, p = _lib.lib(), lambda x: x.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    for j, i in enumerate(range(0, N_ROWS, batch_size)):
        idx = perm[i:i + batch_size].contiguous()
        _lib.check(L.b747_ppo_grad(p(st.theta), od, *(p(b) for b in bufs), p(idx), idx.numel(), CLIP, ENT_COEF, VF_COEF,
                                   p(st.ws), p(st.grad), p(stats[j]), stream), "b747_ppo_grad")
        _lib.check(L.b747_ppo_adam(p(st.theta), p(st.m), p(st.v), p(st.t), p(st.grad), st.theta.numel(), 1.0, MAX_NORM, LR,
                                   BETA1, BETA2, EPS, stream), "b747_ppo_adam")


def _epoch_call(st, od, bufs, perm, batch_size, stats, n_rows=N_ROWS):
    from b747_rl_ctrl_amd import _lib
    L, p = _lib.lib(), lambda x: x.data_ptr()
    return L.b747_ppo_epoch(p(st.theta), od, *(p(b) for b in bufs), p(perm), n_rows, batch_size, CLIP, ENT_COEF, VF_COEF,
                            p(st.ws), p(st.grad), p(st.m), p(st.v), p(st.t), MAX_NORM, LR, BETA1, BETA2, EPS, p(stats),
                            torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("batch_size", [300, 257])      # four minibatches, the last of 124 / 253 rows; odd idx offsets
@pytest.mark.parametrize("od", [3, 5])
def test_two_epoch_calls_against_the_loop_of_two_calls(od, batch_size):
    from b747_rl_ctrl_amd import _lib
    theta0, bufs, perms = _data(od)
    n_mb = -(-N_ROWS // batch_size)
    assert n_mb == 4 and N_ROWS % batch_size not in (0, 1)
    assert theta0.numel() == 128 * od + 8579
    loop, call = _State(theta0, od, n_mb), _State(theta0, od, n_mb)
    for e in range(N_EPOCHS):
        _loop_epoch(loop, od, bufs, perms[e], batch_size, loop.stats[e * n_mb:])
        _lib.check(_epoch_call(call, od, bufs, perms[e], batch_size, call.stats[e * n_mb:]), "b747_ppo_epoch")
    torch.cuda.synchronize()
    assert int(loop.t) == N_EPOCHS * n_mb and not torch.equal(loop.theta, theta0)
    assert bool(torch.isfinite(loop.stats).all()) and bool(torch.isfinite(loop.theta).all())
    for (name, a), b in zip(loop.tensors().items(), call.tensors().values()):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} entries differ"


def test_a_last_minibatch_of_one_row_is_refused_before_anything_runs():
    from b747_rl_ctrl_amd import _lib
    od = 3
    theta0, bufs, perms = _data(od)
    st = _State(theta0, od, 2)
    rc = _epoch_call(st, od, bufs, perms[0], 1023, st.stats)
    assert rc == -1 and b"n_rows % batch_size == 1" in _lib.lib().b747_last_error()
    torch.cuda.synchronize()
    assert torch.equal(st.theta, theta0) and int(st.t) == 0
    assert bool(torch.isnan(st.stats).all()) and bool(torch.isnan(st.grad).all())


# ------------------------------------------------------------------------------------------- PPO.train --
def _env(n=64, seed=3):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, seed=seed)


def _order(epoch, T, n):
    return torch.randperm(T * n, generator=torch.Generator().manual_seed(100 + epoch))


def test_train_with_and_without_the_epoch_call():
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    T = 16
    cfg = PPOConfig(n_steps=T, batch_size=300, n_epochs=2)
    out = []
    for epoch_call in (True, False):
        ppo = PPO(_env(), cfg, seed=5, fused_update=True, epoch_call=epoch_call)
        assert ppo.epoch_call is epoch_call
        ppo.last_obs.copy_(ppo.env.reset())
        ppo.collect_rollouts(T)
        ppo.compute_gae(T)
        stats = ppo.train(T, minibatch_order=_order)
        torch.cuda.synchronize()
        assert int(ppo.upd_t) == 2 * 4                   # 1,024 rows / 300 -> 4 minibatches per epoch
        assert torch.equal(ppo.policy.flat_params(), ppo.flat[:ppo.n_params])
        out.append((ppo.flat[:ppo.n_params].clone(), ppo.upd_m.clone(), ppo.upd_v.clone(), ppo.upd_t.clone(), stats,
                    ppo.adv_buf.clone()))
    a, b = out
    assert torch.equal(a[5], b[5])                       # the same rollout and advantages went in
    for name, x, y in zip(("flat", "upd_m", "upd_v", "upd_t"), a, b):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} entries differ"
    assert set(a[4]) == set(b[4])
    for name in sorted(a[4]):
        assert a[4][name] == b[4][name] and a[4][name] == a[4][name], (name, a[4][name], b[4][name])   # equal, not NaN


def test_the_epoch_call_is_the_default_where_it_applies_and_refused_where_not():
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    cfg = PPOConfig(n_steps=8, batch_size=200, n_epochs=2)
    assert PPO(_env(), cfg, fused_update=True).epoch_call is True
    assert PPO(_env(), cfg).epoch_call is False
    assert PPO(_env(), cfg, fused_update=True, epoch_call=False).epoch_call is False
    with pytest.raises(ValueError, match="fused_update"):
        PPO(_env(), cfg, epoch_call=True)
    with pytest.raises(ValueError, match="data-parallel"):
        PPO(_env(), cfg, fused_update=True, data_parallel=True, epoch_call=True)


def _dp_resolves_to_the_two_calls():
    """In a world-size-1 gloo group (the set-up of tests/test_gpu_ppo_update.py's data-parallel test): with
    data_parallel=True, epoch_call=None resolves to False and epoch_call=True raises"""
    import torch.distributed as dist
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
        try:
            cfg = PPOConfig(n_steps=8, batch_size=200, n_epochs=2)
            dp = PPO(_env(), cfg, seed=2, fused_update=True, data_parallel=True)
            single = PPO(_env(), cfg, seed=2, fused_update=True)
            try:
                PPO(_env(), cfg, seed=2, fused_update=True, data_parallel=True, epoch_call=True)
                raised = False
            except ValueError as e:
                raised = "data-parallel" in str(e)
            return dp.data_parallel is True and dp.epoch_call is False and single.epoch_call is True and raised
        finally:
            dist.destroy_process_group()


def _dp_child(q):
    q.put(_dp_resolves_to_the_two_calls())


def test_data_parallel_keeps_the_two_call_path():
    import torch.distributed as dist
    if not dist.is_initialized():
        assert _dp_resolves_to_the_two_calls()
        return
    import torch.multiprocessing as mp          # the suite's process already holds a group: a child of its own
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_child, args=(q,))
    p.start()
    ok = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0 and ok
