"""The fused PPO minibatch update (b747_ppo_grad + b747_ppo_adam, include/b747.h ABI 12; PPO(fused_update=True)).

The yardstick is torch in fp64: ActorCritic(...).double() with PPO._minibatch's loss, clip_grad_norm_ and
torch.optim.Adam(eps=1e-5).  The same computation in torch fp32 gives the error an fp32 evaluation has against it;
the kernels are a second fp32 evaluation that differs in summation order only (tile order against torch's split-K),
so their error may be at most MARGIN = 4 times that, plus a floor of 1e-7.  The error measure, per parameter tensor
and per statistic, is max |x - x64| / max |x64|.  Nothing is compared against the kernels' own earlier output.
The rollout buffers of the gradient tests are synthetic (a seeded CPU generator): no env is stepped."""
import functools
import math
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 4.0, 1e-7
N_ROWS, CLIP, VF_COEF = 1024, 0.2, 0.5
SEED = 11
STAT_NAMES = ("pg", "vf", "entropy_loss", "clip_fraction", "approx_kl", "abs_a_ratio", "kl_scale", "loss")
PARAM_NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "wa", "ba", "wv", "bv", "log_std")


def _err(x, x64):
    x64 = x64.double()
    return float((x.double() - x64).abs().max() / x64.abs().max())


def _loss_and_stats(policy, obs, act, old_logp, adv, ret, idx, ent_coef):
    """PPO._minibatch's loss and its seven statistics (+ the loss) in the dtype of `policy`"""
    mean, value = policy(obs[idx])
    logp = policy.log_prob(mean, act[idx])
    a = adv[idx]
    a = (a - a.mean()) / (a.std() + 1e-8)
    log_ratio = logp - old_logp[idx]
    ratio = torch.exp(log_ratio)
    pg = -torch.min(a * ratio, a * ratio.clamp(1 - CLIP, 1 + CLIP)).mean()
    vf = ((ret[idx] - value) ** 2).mean()
    ent_loss = -policy.entropy()
    loss = pg + ent_coef * ent_loss + VF_COEF * vf
    st = torch.stack([pg, vf, ent_loss, ((ratio - 1).abs() > CLIP).to(pg.dtype).mean(), ((ratio - 1) - log_ratio).mean(),
                      (a * ratio).abs().mean(), (ratio.abs() + 1 + log_ratio.abs()).mean(), loss]).detach()
    return loss, st, ratio.detach(), a.detach()


def _grads(policy, loss):
    return [g.reshape(-1) for g in torch.autograd.grad(loss, policy.flat_param_list())]


@functools.lru_cache(maxsize=None)
def _data(od):
    """A 1,024-row synthetic rollout for obs_dim `od` (CPU generator: the same numbers everywhere), the policy, and
    old_logp from a perturbed copy of it so that the ratios spread over and beyond the clip range"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    g = torch.Generator().manual_seed(SEED + od)
    torch.manual_seed(SEED + od)
    policy = ActorCritic(od)
    with torch.no_grad():
        for p in policy.parameters():             # off the orthogonal / zero initialisation: every bias non-zero
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
    perm = torch.randperm(N_ROWS, generator=g)
    dev = torch.device("cuda")
    return policy.to(dev), tuple(t.to(dev) for t in (obs, act, old_logp, adv, ret)), perm.to(dev)


def _idx(kind, perm):
    if kind == "b70":                   # one partial wave tile; non-contiguous rows
        return perm[100:170].contiguous()
    if kind == "b257":
        return perm[300:557].contiguous()
    if kind == "perm1024":              # the whole rollout as one shuffled minibatch
        return perm.clone()
    assert kind == "last124"            # 1,024 rows in minibatches of 300: the short last one
    return perm[900:].contiguous()


def _kernel_grad(policy, od, bufs, idx, ent_coef):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    dev = idx.device
    theta = policy.flat_params().contiguous()
    ws = torch.empty(int(L.b747_ppo_update_workspace(od)), dtype=torch.uint8, device=dev)
    grad = torch.full((theta.numel(),), float("nan"), device=dev)
    stats = torch.full((8,), float("nan"), device=dev)
    p = lambda x: x.data_ptr()
    _lib.check(L.b747_ppo_grad(p(theta), od, *(p(b) for b in bufs), p(idx), idx.numel(), CLIP, ent_coef, VF_COEF, p(ws),
                               p(grad), p(stats), torch.cuda.current_stream().cuda_stream), "b747_ppo_grad")
    torch.cuda.synchronize()
    return grad, stats


CASES = [(3, "b70", 0.0), (3, "b257", 0.01), (3, "perm1024", 0.0), (3, "last124", 0.0),
         (5, "b70", 0.0), (5, "b257", 0.0), (5, "perm1024", 0.0), (5, "last124", 0.0), (10, "b257", 0.0)]


@pytest.mark.parametrize("od,kind,ent_coef", CASES)
def test_gradient_and_statistics_against_fp64_autograd(od, kind, ent_coef):
    """Measured on an MI355X (kernel error over the fp32 torch error per tensor, range over the nine cases; DESIGN.md
    11): the weight and hidden-bias gradients 0.06-1.87, the three one-element tensors (action_net.bias, value_net.bias,
    log_std) 0.00-1.00 with an error of at most 5e-8, every statistic at or below torch's error or under the floor.
    The one-element tensors are cancelling sums over the rows of terms in the nets' outputs: with an fp32 forward
    (error ~1e-7 in the output) their error was 1e-7 to 3e-6 and missed the bar whenever torch's own rounding fell
    well, which is why the kernel's forward is fp64."""
    import copy
    policy, bufs, perm = _data(od)
    idx = _idx(kind, perm)
    p64 = copy.deepcopy(policy).double()
    loss64, st64, ratio64, a64 = _loss_and_stats(p64, *(b.double() for b in bufs), idx, ent_coef)
    g64 = _grads(p64, loss64)
    # the inputs cover what they must (asserted on the reference, not on the kernel): ratios inside, above and below
    # the clip range for both advantage signs, and no row on the edge of the clip range
    for sign in (1, -1):
        s = a64 * sign > 0
        assert (s & (ratio64 > 1 + CLIP)).any() and (s & (ratio64 < 1 - CLIP)).any() and (s & ((ratio64 - 1).abs() < CLIP)).any()
    assert float(torch.minimum((ratio64 - (1 + CLIP)).abs(), (ratio64 - (1 - CLIP)).abs()).min()) > 1e-5
    loss32, st32, _, _ = _loss_and_stats(policy, *bufs, idx, ent_coef)
    g32 = _grads(policy, loss32)
    grad, stats = _kernel_grad(policy, od, bufs, idx, ent_coef)
    assert torch.isfinite(grad).all() and torch.isfinite(stats).all()
    bad, off = [], 0
    for name, t32, t64 in zip(PARAM_NAMES, g32, g64):
        e_k, e_t = _err(grad[off:off + t64.numel()], t64), _err(t32, t64)
        off += t64.numel()
        print(f"od {od} {kind} grad {name:8s} kernel {e_k:.3e} torch32 {e_t:.3e} ratio {e_k / max(e_t, 1e-30):.2f}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    assert off == grad.numel()
    for k, name in enumerate(STAT_NAMES):
        if float(st64[k]) == 0.0:
            assert float(stats[k]) == 0.0, name
            continue
        e_k, e_t = _err(stats[k:k + 1], st64[k:k + 1]), _err(st32[k:k + 1], st64[k:k + 1])
        print(f"od {od} {kind} stat {name:13s} kernel {e_k:.3e} torch32 {e_t:.3e}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    assert not bad, bad


def test_two_calls_give_the_same_bits():
    policy, bufs, perm = _data(3)
    a = _kernel_grad(policy, 3, bufs, perm, 0.01)
    b = _kernel_grad(policy, 3, bufs, perm, 0.01)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _adam_kernel(theta, m, v, t, grad, scale, max_norm, lr):
    from b747_rl_ctrl_amd import _lib
    p = lambda x: x.data_ptr()
    _lib.check(_lib.lib().b747_ppo_adam(p(theta), p(m), p(v), p(t), p(grad), theta.numel(), scale, max_norm, lr, 0.9,
                                        0.999, 1e-5, torch.cuda.current_stream().cuda_stream), "b747_ppo_adam")


def test_adam_and_clip_against_torch():
    dev, max_norm, lr = torch.device("cuda"), 0.5, 3e-4
    P = 2 * (3 * 64 + 64 + 64 * 64 + 64) + 65 + 65 + 1     # the obs_dim 3 policy's parameters
    g = torch.Generator().manual_seed(SEED)
    theta0 = (0.1 * torch.randn(P, generator=g)).to(dev)
    big, small = torch.randn(P, generator=g).to(dev), (1e-3 * torch.randn(P, generator=g)).to(dev)
    assert float(big.double().norm()) > max_norm > float(small.double().norm())     # one clipped, one not
    seq = [big, small, big]

    def torch_run(dtype):
        prm = torch.nn.Parameter(theta0.to(dtype).clone())
        opt = torch.optim.Adam([prm], lr=lr, eps=1e-5)
        for gr in seq:
            prm.grad = gr.to(dtype).clone()
            torch.nn.utils.clip_grad_norm_([prm], max_norm)
            opt.step()
        st = opt.state[prm]
        return prm.detach(), st["exp_avg"], st["exp_avg_sq"]

    ref64, ref32 = torch_run(torch.float64), torch_run(torch.float32)
    theta, m, v = theta0.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    t = torch.zeros(1, dtype=torch.int64, device=dev)
    for gr in seq:
        keep = gr.clone()
        _adam_kernel(theta, m, v, t, gr, 1.0, max_norm, lr)
        assert torch.equal(gr, keep)                       # the gradient is the caller's: not clipped in place
    assert int(t) == 3
    for name, x, x32, x64 in zip(("theta", "m", "v"), (theta, m, v), ref32, ref64):
        e_k, e_t = _err(x, x64), _err(x32, x64)
        print(f"adam {name} kernel {e_k:.3e} torch32 {e_t:.3e}")
        assert e_k <= MARGIN * e_t + FLOOR, (name, e_k, e_t)
    # grad_scale = 0.5 is halving the gradient first
    outs = []
    for gr, scale in ((big, 0.5), (0.5 * big, 1.0)):
        th, m1, v1 = theta0.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev)
        t1 = torch.zeros(1, dtype=torch.int64, device=dev)
        _adam_kernel(th, m1, v1, t1, gr, scale, 100.0, lr)          # (|g| / 2 < 100: unclipped either way)
        _adam_kernel(th, m1, v1, t1, gr, scale, max_norm, lr)
        outs.append((th, m1, v1))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------- train() --
def _env(n=64, seed=3):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST, tk=0.3, seed=seed)


T_TRAIN = 16
ROLLOUT_BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf")


def _order(epoch, T, n):
    return torch.randperm(T * n, generator=torch.Generator().manual_seed(100 + epoch))


def _train_fp64(ppo, start, T):
    """PPO.train on ppo's rollout in fp64 torch from the parameters `start`: (final parameters, statistics)"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    c, n = ppo.cfg, ppo.env.n
    N = T * n
    pol = ActorCritic(ppo.env.obs_dim).to(ppo.env.device).double()
    pol.load_state_dict({k: v.double() for k, v in start.items()})
    opt = torch.optim.Adam(pol.parameters(), lr=c.learning_rate, eps=1e-5)
    views = tuple(b[:T].reshape(N, *b.shape[2:]).double() for b in (ppo.obs_buf, ppo.act_buf, ppo.logp_buf, ppo.adv_buf,
                                                                   ppo.ret_buf))
    n_mb = -(-N // c.batch_size)
    rows = []
    for epoch in range(c.n_epochs):
        perm = _order(epoch, T, n).to(ppo.env.device)
        for i in range(0, N, c.batch_size):
            loss, st, _, _ = _loss_and_stats(pol, *views, perm[i:i + c.batch_size], c.ent_coef)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), c.max_grad_norm)
            opt.step()
            rows.append(st)
    rows = torch.stack(rows)
    mean = rows.mean(0).tolist()
    v, r = ppo.val_buf[:T].reshape(N).double(), views[4]
    stats = {"entropy_loss": mean[2], "policy_gradient_loss": mean[0], "value_loss": mean[1],
             "approx_kl": float(rows[(c.n_epochs - 1) * n_mb:, 4].mean()), "clip_fraction": mean[3],
             "loss": float(rows[-1, 7]), "explained_variance": float(1 - (r - v).var(unbiased=False) / r.var(unbiased=False)),
             "std": float(pol.log_std.exp().mean()), "pg_term_scale": mean[5],
             "kl_term_scale": float(rows[(c.n_epochs - 1) * n_mb:, 6].mean())}
    stats["policy_loss"] = stats["policy_gradient_loss"]
    return pol, stats


def test_train_end_to_end_against_the_default_path_and_fp64():
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    T = T_TRAIN
    cfg = PPOConfig(n_steps=T, batch_size=300, n_epochs=2)
    pf = PPO(_env(), cfg, seed=5, fused_update=True)
    pd = PPO(_env(), cfg, seed=5)
    assert pf.fused_update and not pd.fused_update
    pf.last_obs.copy_(pf.env.reset())
    pf.collect_rollouts(T)
    pf.compute_gae(T)
    for name in ROLLOUT_BUFS:                      # the same rollout through all three paths
        getattr(pd, name).copy_(getattr(pf, name))
    start = {k: v.clone() for k, v in pf.policy.state_dict().items()}
    assert all(torch.equal(v, pd.policy.state_dict()[k]) for k, v in start.items())
    p64, s64 = _train_fp64(pf, start, T)
    sf = pf.train(T, minibatch_order=_order)
    sd = pd.train(T, minibatch_order=_order)
    assert set(sf) == set(sd) == set(s64)
    # every other method sees the new policy: the modules hold the flat master copy
    assert torch.equal(pf.policy.flat_params(), pf.flat[:pf.n_params])
    assert int(pf.upd_t) == 2 * 4 and not pf.opt.state           # 1,024 rows / 300 -> 4 minibatches per epoch
    bad = []
    for name, xf, xd, x64 in zip(PARAM_NAMES, pf.policy.flat_param_list(), pd.policy.flat_param_list(),
                                 p64.flat_param_list()):
        e_f, e_d = _err(xf.detach(), x64.detach()), _err(xd.detach(), x64.detach())
        print(f"train param {name:8s} fused {e_f:.3e} default {e_d:.3e}")
        if not e_f <= MARGIN * e_d + FLOOR:
            bad.append((name, e_f, e_d))
    for name in sorted(s64):
        assert math.isfinite(sf[name]), name
        if s64[name] == 0.0:
            assert sf[name] == 0.0, name
            continue
        e_f, e_d = abs(sf[name] - s64[name]) / abs(s64[name]), abs(sd[name] - s64[name]) / abs(s64[name])
        print(f"train stat {name:22s} fused {e_f:.3e} default {e_d:.3e}")
        if not e_f <= MARGIN * e_d + FLOOR:
            bad.append((name, e_f, e_d))
    assert not bad, bad


def test_learn_runs_with_the_fused_update():
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    ppo = PPO(_env(512), PPOConfig(n_steps=32, batch_size=4096, n_epochs=2), seed=0, fused_update=True)
    before = ppo.policy.flat_params().clone()
    hist = ppo.learn(2)
    assert len(hist) == 2 and all(math.isfinite(v) for h in hist for v in h.values())
    assert not torch.equal(before, ppo.policy.flat_params())
    with pytest.raises(ValueError, match="fused=True"):
        PPO(_env(), PPOConfig(n_steps=8, batch_size=256), fused=False, fused_update=True)


# ------------------------------------------------------------------------------- data-parallel glue --
def _fill(ppo, T, seed):
    g = torch.Generator().manual_seed(seed)
    dev = ppo.env.device
    with torch.no_grad():
        ppo.obs_buf.copy_(torch.randn(ppo.obs_buf.shape, generator=g))
        mean, _ = ppo.policy(ppo.obs_buf)
        ppo.act_buf.copy_(mean + torch.randn(ppo.act_buf.shape, generator=g).to(dev))
        ppo.logp_buf.copy_(ppo.policy.log_prob(mean, ppo.act_buf) + 0.1 * torch.randn(ppo.logp_buf.shape, generator=g).to(dev))
        ppo.adv_buf.copy_(torch.randn(ppo.adv_buf.shape, generator=g))
        ppo.ret_buf.copy_(torch.randn(ppo.ret_buf.shape, generator=g))
        ppo.val_buf.copy_(torch.randn(ppo.val_buf.shape, generator=g))


def _dp_equal_to_single():
    """In a world-size-1 gloo group: fused_update with data_parallel (the all-reduce between the two calls) ends on
    the same bits as without"""
    import torch.distributed as dist
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
        try:
            out = []
            for dp in (True, False):
                ppo = PPO(_env(), PPOConfig(n_steps=8, batch_size=200, n_epochs=2), seed=2, fused_update=True,
                          data_parallel=dp)
                assert ppo.data_parallel is dp
                _fill(ppo, 8, seed=9)
                ppo.train(8, minibatch_order=_order)
                out.append(ppo.policy.flat_params().cpu())
            return bool(torch.equal(out[0], out[1])) and bool(torch.isfinite(out[0]).all())
        finally:
            dist.destroy_process_group()


def _dp_child(q):
    q.put(_dp_equal_to_single())


def test_data_parallel_glue_in_a_world_of_one():
    import torch.distributed as dist
    if not dist.is_initialized():
        assert _dp_equal_to_single()
        return
    import torch.multiprocessing as mp          # the suite's process already holds a group: a child of its own
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_child, args=(q,))
    p.start()
    ok = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0 and ok
