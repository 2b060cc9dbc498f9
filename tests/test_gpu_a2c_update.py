"""The fused A2C update (b747_a2c_grad, b747_ppo_rmsprop, b747_a2c_update; include/b747.h).

The yardstick and the margins are tests/test_gpu_ppo_update.py's: torch in fp64 -- ActorCritic(...).double() with SB3 1.4
A2C.train's loss mean(-A logp) + ent_coef (-entropy) + vf_coef mean((ret - value)^2), clip_grad_norm_ and
torch.optim.RMSprop (or, for the TF-like flavour, a transcription of its formula written here).  The same computation
in torch fp32 gives the error an fp32 evaluation has against it; the kernels are a second fp32 evaluation that differs
in summation order only, so their error may be at most MARGIN = 4 times that, plus a floor of 1e-7.  The error measure,
per parameter tensor and per statistic, is max |x - x64| / max |x64|.  Nothing is compared against the kernels' own
earlier output.  The rollout buffers are synthetic (a seeded CPU generator): no env is stepped."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 4.0, 1e-7
N_ROWS, N_GRID, VF_COEF = 1024, 20000, 0.5
SEED = 23
STAT_NAMES = ("policy_loss", "value_loss", "entropy_loss", "slot3", "slot4", "abs_a_logp", "slot6", "loss")
PARAM_NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "wa", "ba", "wv", "bv", "log_std")
P3 = 2 * (3 * 64 + 64 + 64 * 64 + 64) + 65 + 65 + 1     # the obs_dim 3 policy's parameters


def _err(x, x64):
    x64 = x64.double()
    return float((x.double() - x64).abs().max() / x64.abs().max())


def _loss_and_stats(policy, obs, act, adv, ret, idx, normalize, ent_coef):
    """A2C.train's loss and the statistics row of b747_a2c_grad in the dtype of `policy`"""
    mean, value = policy(obs[idx])
    logp = policy.log_prob(mean, act[idx])
    a = adv[idx]
    if normalize:
        a = (a - a.mean()) / (a.std() + 1e-8)
    pl = -(a * logp).mean()
    vf = ((ret[idx] - value) ** 2).mean()
    ent_loss = -policy.entropy()
    loss = pl + ent_coef * ent_loss + VF_COEF * vf
    zero = torch.zeros_like(pl)
    st = torch.stack([pl, vf, ent_loss, zero, zero, (a * logp).abs().mean(), zero, loss]).detach()
    return loss, st, a.detach()


def _grads(policy, loss):
    return [g.reshape(-1) for g in torch.autograd.grad(loss, policy.flat_param_list())]


@functools.lru_cache(maxsize=None)
def _data(od, n_rows=N_ROWS):
    """An n_rows-row synthetic rollout for obs_dim `od` (CPU generator: the same numbers everywhere) and the policy that
    drew its actions"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    g = torch.Generator().manual_seed(SEED + od + n_rows)
    torch.manual_seed(SEED + od)
    policy = ActorCritic(od)
    with torch.no_grad():
        for p in policy.parameters():             # off the orthogonal / zero initialisation: every bias non-zero
            p.add_(0.05 * torch.randn(p.shape, generator=g))
        policy.log_std.fill_(-0.3)
    obs = torch.randn(n_rows, od, generator=g)
    with torch.no_grad():
        mean, _ = copy.deepcopy(policy).double()(obs.double())
        act = (mean + policy.log_std.double().exp() * torch.randn(n_rows, 1, generator=g, dtype=torch.float64)).float()
    adv = 0.3 + 1.5 * torch.randn(n_rows, generator=g)
    ret = torch.randn(n_rows, generator=g)
    perm = torch.randperm(n_rows, generator=g)
    dev = torch.device("cuda")
    return policy.to(dev), tuple(t.to(dev) for t in (obs, act, adv, ret)), perm.to(dev)


# kind -> (the rows as the kernel gets them: an index tensor or None = the first `batch` rows in order, batch)
def _rows(kind, perm):
    n = perm.numel()
    if kind == "b1":
        return perm[5:6].contiguous(), 1
    if kind in ("b31", "b32", "b33"):           # the tile edge
        b = int(kind[1:])
        return perm[:b].contiguous(), b
    if kind == "b70":                           # one partial wave tile; shuffled, non-contiguous rows
        return perm[100:170].contiguous(), 70
    if kind == "b257":
        return perm[300:557].contiguous(), 257
    if kind == "null":                          # the whole buffer, no index array
        return None, n
    assert kind == "perm"                       # the whole buffer, shuffled
    return perm.clone(), n


@functools.lru_cache(maxsize=None)
def _reference(od, n_rows, kind, normalize, ent_coef):
    """(fp64 gradient, fp64 statistics, fp64 advantages, fp32 gradient, fp32 statistics) for the case, computed once"""
    policy, bufs, perm = _data(od, n_rows)
    idx, batch = _rows(kind, perm)
    if idx is None:
        idx = torch.arange(batch, device=perm.device)
    p64 = copy.deepcopy(policy).double()
    loss64, st64, a64 = _loss_and_stats(p64, *(b.double() for b in bufs), idx, normalize, ent_coef)
    g64 = _grads(p64, loss64)
    loss32, st32, _ = _loss_and_stats(policy, *bufs, idx, normalize, ent_coef)
    g32 = _grads(policy, loss32)
    return g64, st64, a64, g32, st32


def _kernel_grad(od, n_rows, kind, normalize, ent_coef):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    policy, bufs, perm = _data(od, n_rows)
    idx, batch = _rows(kind, perm)
    dev = perm.device
    theta = policy.flat_params().contiguous()
    ws = torch.empty(int(L.b747_ppo_update_workspace(od)), dtype=torch.uint8, device=dev)
    grad = torch.full((theta.numel(),), float("nan"), device=dev)
    stats = torch.full((8,), float("nan"), device=dev)
    p = lambda x: x.data_ptr()
    _lib.check(L.b747_a2c_grad(p(theta), od, *(p(b) for b in bufs), None if idx is None else p(idx), batch, int(normalize),
                               ent_coef, VF_COEF, p(ws), p(grad), p(stats), torch.cuda.current_stream().cuda_stream),
               "b747_a2c_grad")
    torch.cuda.synchronize()
    return grad, stats


KINDS = ("b31", "b32", "b33", "b70", "b257", "null", "perm")
ENT = {"b33": 0.01, "b257": 0.01, "null": 0.01, "perm": 0.01}      # at obs_dim 3 (the other kinds: 0); at 5 the reverse
CASES = [(od, N_ROWS, "b1", False, e) for od, e in ((3, 0.0), (5, 0.01))] \
    + [(od, N_ROWS, k, nrm, ENT.get(k, 0.0) if od == 3 else 0.01 - ENT.get(k, 0.0))
       for od in (3, 5) for k in KINDS for nrm in (False, True)] \
    + [(10, N_ROWS, "b257", True, 0.0),
       (3, N_GRID, "null", False, 0.01), (3, N_GRID, "null", True, 0.0)]      # 625 tiles on 256 workgroups: the tile loop


@pytest.mark.parametrize("od,n_rows,kind,normalize,ent_coef", CASES)
def test_gradient_and_statistics_against_fp64_autograd(od, n_rows, kind, normalize, ent_coef):
    """Measured on an MI355X (kernel error over the fp32 torch error per tensor, range over the 33 cases): the weight and
    hidden-bias gradients 0.01-2.23 with a kernel error of at most 2.1e-6; the three one-element tensors
    (action_net.bias, value_net.bias, log_std) 0.00-1.00 with a kernel error of at most 1.1e-7; the statistics at or
    below torch's error but for the loss (up to 7.2 times a torch error that fell under 1.3e-8; kernel error at most
    9.3e-8, under the floor).  No case used more than 0.51 of its bound."""
    # "null" and "perm" are the same set of rows: ONE reference, in the buffer's order, for both
    g64, st64, a64, g32, st32 = _reference(od, n_rows, "null" if kind == "perm" else kind, normalize, ent_coef)
    if a64.numel() > 1:      # asserted on the reference, not on the kernel: advantages of both signs
        assert bool((a64 > 0).any()) and bool((a64 < 0).any())
    grad, stats = _kernel_grad(od, n_rows, kind, normalize, ent_coef)
    assert torch.isfinite(grad).all() and torch.isfinite(stats).all()
    tag = f"od {od} {kind} n{n_rows} norm {int(normalize)} ent {ent_coef}"
    bad, off = [], 0
    for name, t32, t64 in zip(PARAM_NAMES, g32, g64):
        e_k, e_t = _err(grad[off:off + t64.numel()], t64), _err(t32, t64)
        off += t64.numel()
        print(f"{tag} grad {name:8s} kernel {e_k:.3e} torch32 {e_t:.3e} ratio {e_k / max(e_t, 1e-30):.2f}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    assert off == grad.numel()
    for k, name in enumerate(STAT_NAMES):
        if float(st64[k]) == 0.0:
            assert float(stats[k]) == 0.0, name
            continue
        e_k, e_t = _err(stats[k:k + 1], st64[k:k + 1]), _err(st32[k:k + 1], st64[k:k + 1])
        print(f"{tag} stat {name:13s} kernel {e_k:.3e} torch32 {e_t:.3e}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    assert not bad, bad


def test_two_calls_give_the_same_bits():
    a = _kernel_grad(3, N_ROWS, "perm", True, 0.01)
    b = _kernel_grad(3, N_ROWS, "perm", True, 0.01)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _rmsprop_kernel(theta, sq, t, grad, scale, max_norm, lr, alpha, eps, tf_like):
    from b747_rl_ctrl_amd import _lib
    p = lambda x: x.data_ptr()
    _lib.check(_lib.lib().b747_ppo_rmsprop(p(theta), p(sq), p(t), p(grad), theta.numel(), scale, max_norm, lr, alpha, eps,
                                           int(tf_like), torch.cuda.current_stream().cuda_stream), "b747_ppo_rmsprop")


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop", "rmsprop_tf"])
def test_update_gives_the_bits_of_grad_then_the_optimiser(optimizer):
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.ppo import A2C_OPTIMIZERS
    L = _lib.lib()
    od, lr, max_norm, alpha = 3, 7e-4, 0.5, 0.99
    eps = {"adam": 1e-5, "rmsprop": 1e-5, "rmsprop_tf": 1e-9}[optimizer]
    policy, bufs, perm = _data(od)
    dev = perm.device
    p = lambda x: x.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for one_call in (False, True):
        theta = policy.flat_params().contiguous()
        ws = torch.empty(int(L.b747_ppo_update_workspace(od)), dtype=torch.uint8, device=dev)
        grad, stats = torch.full((P3,), float("nan"), device=dev), torch.full((8,), float("nan"), device=dev)
        s0 = torch.full((P3,), 1.0 if optimizer == "rmsprop_tf" else 0.0, device=dev)
        s1 = torch.zeros(P3, device=dev)
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        rows = (p(theta), od, *(p(b) for b in bufs), p(perm), perm.numel(), 1, 0.01, VF_COEF, p(ws), p(grad), p(stats))
        for _ in range(2):                                   # two steps: the second from a non-trivial state
            if one_call:
                _lib.check(L.b747_a2c_update(*rows, A2C_OPTIMIZERS.index(optimizer), p(s0),
                                             p(s1) if optimizer == "adam" else None, p(t), max_norm, lr, alpha, eps,
                                             stream), "b747_a2c_update")
                continue
            _lib.check(L.b747_a2c_grad(*rows, stream), "b747_a2c_grad")
            if optimizer == "adam":
                _lib.check(L.b747_ppo_adam(p(theta), p(s0), p(s1), p(t), p(grad), P3, 1.0, max_norm, lr, 0.9, 0.999, eps,
                                           stream), "b747_ppo_adam")
            else:
                _rmsprop_kernel(theta, s0, t, grad, 1.0, max_norm, lr, alpha, eps, optimizer == "rmsprop_tf")
        torch.cuda.synchronize()
        assert int(t) == 2 and torch.isfinite(theta).all() and not torch.equal(theta, policy.flat_params())
        outs.append((theta, grad, stats, s0, s1, t))
    for name, a, b in zip(("theta", "grad", "stats", "state0", "state1", "t"), *outs):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("tf_like", [False, True])
def test_rmsprop_and_clip_against_torch(tf_like):
    """Three steps on a clipped, an unclipped and a clipped gradient.  The torch flavour against torch.optim.RMSprop; the
    TF-like flavour against a transcription of its formula (epsilon inside the root, state starting at ones).
    Measured on an MI355X: theta 8.3e-8 / 8.4e-8 (torch flavour / TF-like), equal to the fp32 run's error; sq 9.7e-8 /
    6.7e-8 against the fp32 run's 1.8e-7 / 1.7e-7."""
    dev, max_norm, lr, alpha = torch.device("cuda"), 0.5, 7e-4, 0.99
    eps = 1e-9 if tf_like else 1e-5
    g = torch.Generator().manual_seed(SEED)
    theta0 = (0.1 * torch.randn(P3, generator=g)).to(dev)
    big, small = torch.randn(P3, generator=g).to(dev), (1e-3 * torch.randn(P3, generator=g)).to(dev)
    assert float(big.double().norm()) > max_norm > float(small.double().norm())     # one clipped, one not
    seq = [big, small, big]

    def torch_run(dtype):
        prm = torch.nn.Parameter(theta0.to(dtype).clone())
        opt = torch.optim.RMSprop([prm], lr=lr, alpha=alpha, eps=eps)
        for gr in seq:
            prm.grad = gr.to(dtype).clone()
            torch.nn.utils.clip_grad_norm_([prm], max_norm)
            opt.step()
        return prm.detach(), opt.state[prm]["square_avg"]

    def tf_run(dtype):
        th, sq = theta0.to(dtype).clone(), torch.ones(P3, dtype=dtype, device=dev)
        for gr in seq:
            gc = gr.to(dtype)
            gc = gc * torch.clamp(max_norm / (gc.norm() + 1e-6), max=1.0)      # clip_grad_norm_
            sq = alpha * sq + (1 - alpha) * gc * gc
            th = th - lr * gc / torch.sqrt(sq + eps)
        return th, sq

    run = tf_run if tf_like else torch_run
    ref64, ref32 = run(torch.float64), run(torch.float32)
    theta, sq = theta0.clone(), torch.full((P3,), 1.0 if tf_like else 0.0, device=dev)
    t = torch.zeros(1, dtype=torch.int64, device=dev)
    for gr in seq:
        keep = gr.clone()
        _rmsprop_kernel(theta, sq, t, gr, 1.0, max_norm, lr, alpha, eps, tf_like)
        assert torch.equal(gr, keep)                       # the gradient is the caller's: not clipped in place
    assert int(t) == 3
    for name, x, x32, x64 in zip(("theta", "sq"), (theta, sq), ref32, ref64):
        e_k, e_t = _err(x, x64), _err(x32, x64)
        print(f"rmsprop tf_like {int(tf_like)} {name} kernel {e_k:.3e} torch32 {e_t:.3e}")
        assert e_k <= MARGIN * e_t + FLOOR, (name, e_k, e_t)
    # grad_scale = 0.5 is halving the gradient first
    outs = []
    for gr, scale in ((big, 0.5), (0.5 * big, 1.0)):
        th, s1 = theta0.clone(), torch.full((P3,), 1.0 if tf_like else 0.0, device=dev)
        t1 = torch.zeros(1, dtype=torch.int64, device=dev)
        _rmsprop_kernel(th, s1, t1, gr, scale, 100.0, lr, alpha, eps, tf_like)      # (|g| / 2 < 100: unclipped either way)
        _rmsprop_kernel(th, s1, t1, gr, scale, max_norm, lr, alpha, eps, tf_like)
        outs.append((th, s1))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
