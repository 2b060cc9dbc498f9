"""k_ppo_grad<OD> / k_ppo_reduce (csrc/b747_ppo_update.h) at the full grid, in the tile loop's later iterations, at the
tile and workgroup boundaries and for every obs_dim -- the shapes tests/test_gpu_ppo_update.py's 1,024-row rollout
does not reach.

Geometry (launch_ppo_grad, csrc/b747_ppo_update.hip), from kUpdTile = 32 rows per wave tile and kUpdMaxWG = 256:
tiles = ceil(batch / 32), n_wg = min(256, (tiles + 1) // 2).  A workgroup has two wave slots per net (waves 0 / 1 the
policy net, 2 / 3 the value net); slot s = 2 wg + (wave & 1) of the 2 n_wg slots walks the tiles s, s + 2 n_wg, ...:
trips(s) = ceil((tiles - s) / (2 n_wg)) for s < tiles and 0 (the wave is idle) otherwise.  The last tile has
batch - 32 (tiles - 1) valid rows.  _geometry() restates this and GEOMETRY holds what it gives for the cases:

    batch   tiles  n_wg  slots by trip count       last tile
        2       1     1  one idle, one x1           2 rows (30 lanes past the minibatch; waves 1 / 3 idle)
   31, 32       1     1  one idle, one x1          31, 32 rows
       33       2     1  two x1                     1 row  (the second wave's tile)
       64       2     1  two x1                    32 rows
       65       3     2  one idle, three x1         1 row  (the last workgroup's second wave idle)
   16,352     511   256  one idle, 511 x1          32 rows (first full grid)
   16,384     512   256  512 x1                    32 rows
   16,385     513   256  511 x1, one x2             1 row  (one wave pair runs a second tile)
   16,454     515   256  509 x1, three x2           6 rows
   32,869   1,028   256  508 x2, four x3            5 rows

If kUpdTile, kUpdMaxWG or the launcher's n_wg change, test_the_cases_reach_what_they_are_for fails and the cases need
revisiting.

The yardstick is tests/test_gpu_ppo_update.py's: ActorCritic(od).double() with PPO._minibatch's loss under fp64
autograd, the error measure max |x - x64| / max |x64| per parameter tensor and per statistic, the bar
e_kernel <= MARGIN e_t + FLOOR with MARGIN = 4 and FLOOR = 1e-7.  e_t, the error of an fp32 torch evaluation against the
same fp64 result, is the maximum over three row orders (idx as given and two seeded shuffles of it): the loss and its
gradient do not depend on the row order in exact arithmetic, so all three estimate the same quantity, and the maximum
keeps the bar from resting on one draw whose rounding fell well.  The kernel runs once, on idx as given.  Nothing is
compared with the kernels' own earlier output except where "the same bits" is the claim.

Inputs: a 40,000-row synthetic pool per od (the recipe of test_gpu_ppo_update._data from a CPU generator seeded
SEED + od + 1000), then one repair pass on the reference only: old_logp of every row whose fp64 ratio is within 1e-4
of 1 +- CLIP is raised by 0.01.  After it no row of the pool is within 1e-4 of a clip edge (asserted, with a cap of
0.1 % of the pool on the rows touched), so that holds for every minibatch, and the clip fraction -- an fp64 count in
the kernel, whose fp64 forward is ~1e-15 from the reference -- is exact.  Minibatches are slices of one permutation
of the pool: rows scattered over it, odd offsets."""
import collections
import copy
import functools
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 4.0, 1e-7
POOL, CLIP, VF_COEF = 40_000, 0.2, 0.5
EDGE = 1e-4                       # no pool row's fp64 ratio is this close to 1 +- CLIP
SEED = 11
MAX_NORM, LR, EPS = 0.5, 3e-4, 1e-5
K_UPD_TILE, K_UPD_MAX_WG = 32, 256
GUARD, WS_TAIL, WS_GUARD = -12345.0, 256, 0xA5
STAT_NAMES = ("pg", "vf", "entropy_loss", "clip_fraction", "approx_kl", "abs_a_ratio", "kl_scale", "loss")
PARAM_NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "wa", "ba", "wv", "bv", "log_std")
ALL_OD = (3, 5, 7, 8, 10)

# batch: (tiles, n_wg, {trip count: wave slots}, valid rows of the last tile)
GEOMETRY = {
    2: (1, 1, {0: 1, 1: 1}, 2),
    31: (1, 1, {0: 1, 1: 1}, 31),
    32: (1, 1, {0: 1, 1: 1}, 32),
    33: (2, 1, {1: 2}, 1),
    64: (2, 1, {1: 2}, 32),
    65: (3, 2, {0: 1, 1: 3}, 1),
    16_352: (511, 256, {0: 1, 1: 511}, 32),
    16_384: (512, 256, {1: 512}, 32),
    16_385: (513, 256, {1: 511, 2: 1}, 1),
    16_454: (515, 256, {1: 509, 2: 3}, 6),
    32_869: (1028, 256, {2: 508, 3: 4}, 5),
}
# where in the permutation each minibatch starts (odd: idx is not aligned to anything)
START = {2: 7, 31: 101, 32: 203, 33: 307, 64: 401, 65: 503, 16_352: 1001, 16_384: 2003, 16_385: 3001, 16_454: 20_001,
         32_869: 1237}
CASES = ([(od, b, 0.01 if (od, b) == (7, 16_454) else 0.0) for b in (2, 33, 65, 16_454) for od in ALL_OD]
         + [(od, b, 0.0) for b in (31, 32, 64, 16_352, 16_384, 16_385, 32_869) for od in (3, 10)])


def _geometry(batch):
    tiles = -(-batch // K_UPD_TILE)
    n_wg = min(K_UPD_MAX_WG, (tiles + 1) // 2)
    trips = collections.Counter(len(range(s, tiles, 2 * n_wg)) for s in range(2 * n_wg))
    return tiles, n_wg, dict(trips), batch - K_UPD_TILE * (tiles - 1)


def test_the_cases_reach_what_they_are_for():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "b747_rl_ctrl_amd", "csrc", "b747_ppo_update.h")) as f:
        header = f.read()
    with open(os.path.join(root, "b747_rl_ctrl_amd", "csrc", "b747_ppo_update.hip")) as f:
        launcher = f.read()
    assert int(re.search(r"constexpr int kUpdTile = (\d+);", header).group(1)) == K_UPD_TILE
    assert int(re.search(r"constexpr int kUpdMaxWG = (\d+);", header).group(1)) == K_UPD_MAX_WG
    launcher = re.sub(r"\s+", "", launcher)
    assert "tiles=(batch+kUpdTile-1)/kUpdTile,want=(tiles+1)/2;" in launcher
    assert "n_wg=(int)(want<kUpdMaxWG?want:kUpdMaxWG);" in launcher
    assert {b for _, b, _ in CASES} == set(GEOMETRY) == set(START)
    for batch, want in GEOMETRY.items():
        assert _geometry(batch) == want, batch
        assert START[batch] % 2 == 1 and START[batch] + batch <= POOL and batch != 65_536
    for od in ALL_OD:
        assert {b for o, b, _ in CASES if o == od} >= {2, 33, 65, 16_454}
    for od in (3, 10):
        assert {b for o, b, _ in CASES if o == od} == set(GEOMETRY)
    assert sum(1 for _, _, e in CASES if e != 0.0) == 1


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


def _edge_distance(ratio):
    return torch.minimum((ratio - (1 + CLIP)).abs(), (ratio - (1 - CLIP)).abs())


@functools.lru_cache(maxsize=None)
def _pool(od):
    """On the CPU (the same numbers everywhere): the policy, the 40,000-row pool (obs, act, old_logp, adv, ret) after
    the repair pass, the permutation, and how many rows the repair touched.  The input conditions that hold pool-wide
    are asserted here, on the fp64 reference."""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    g = torch.Generator().manual_seed(SEED + od + 1000)
    torch.manual_seed(SEED + od)                  # (the initialisation is test_gpu_ppo_update._data's)
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
    obs = torch.randn(POOL, od, generator=g)
    with torch.no_grad():
        mean_old, _ = old.double()(obs.double())
        act = (mean_old + old.log_std.exp() * torch.randn(POOL, 1, generator=g, dtype=torch.float64)).float()
        old_logp = old.log_prob(mean_old, act.double()).float()
    adv = 0.3 + 1.5 * torch.randn(POOL, generator=g)
    ret = torch.randn(POOL, generator=g)
    perm = torch.randperm(POOL, generator=g)
    p64 = copy.deepcopy(policy).double()

    def ratios():
        with torch.no_grad():
            mean, _ = p64(obs.double())
            return torch.exp(p64.log_prob(mean, act.double()) - old_logp.double())

    near = _edge_distance(ratios()) <= EDGE
    old_logp[near] += 0.01
    ratio = ratios()
    assert float(_edge_distance(ratio).min()) > EDGE
    assert int(near.sum()) <= POOL // 1000
    return policy, (obs, act, old_logp, adv, ret), perm, int(near.sum())


@functools.lru_cache(maxsize=None)
def _data(od):
    policy, bufs, perm, _ = _pool(od)
    dev = torch.device("cuda")
    return copy.deepcopy(policy).to(dev), tuple(t.to(dev) for t in bufs), perm.to(dev)


def _idx(perm, batch):
    return perm[START[batch]:START[batch] + batch].contiguous()


def _workspace(od):
    """The workspace with every byte 0xFF (NaN in both float widths: a partial this call did not write shows) and
    WS_TAIL guard bytes behind it"""
    from b747_rl_ctrl_amd import _lib
    n = int(_lib.lib().b747_ppo_update_workspace(od))
    ws = torch.full((n + WS_TAIL,), 0xFF, dtype=torch.uint8, device="cuda")
    ws[n:] = WS_GUARD
    return ws


def _kernel_grad(policy, od, bufs, idx, ent_coef, ws=None):
    """b747_ppo_grad into NaN-filled grad / stats with one guard element each and a guarded workspace: (grad[P],
    stats[8]), finite, and nothing written past any of the three"""
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    dev = idx.device
    theta = policy.flat_params().contiguous()
    P, n_ws = theta.numel(), int(L.b747_ppo_update_workspace(od))
    assert P == 128 * od + 8579
    ws = _workspace(od) if ws is None else ws
    assert ws.numel() == n_ws + WS_TAIL
    grad = torch.full((P + 1,), float("nan"), device=dev)
    stats = torch.full((8 + 1,), float("nan"), device=dev)
    grad[P] = GUARD
    stats[8] = GUARD
    p = lambda x: x.data_ptr()
    _lib.check(L.b747_ppo_grad(p(theta), od, *(p(b) for b in bufs), p(idx), idx.numel(), CLIP, ent_coef, VF_COEF, p(ws),
                               p(grad), p(stats), torch.cuda.current_stream().cuda_stream), "b747_ppo_grad")
    torch.cuda.synchronize()
    assert float(grad[P]) == GUARD and float(stats[8]) == GUARD, "written past grad[P] / stats[8]"
    assert bool((ws[n_ws:] == WS_GUARD).all()), "written past the workspace"
    assert bool(torch.isfinite(grad[:P]).all()) and bool(torch.isfinite(stats[:8]).all())
    return grad[:P].clone(), stats[:8].clone()


def _row_orders(idx):
    """idx and two seeded shuffles of it"""
    g = torch.Generator().manual_seed(SEED + 2000 + idx.numel())
    return [idx] + [idx[torch.randperm(idx.numel(), generator=g).to(idx.device)].contiguous() for _ in range(2)]


@pytest.mark.parametrize("od,batch,ent_coef", CASES)
def test_gradient_statistics_row_count_and_bounds(od, batch, ent_coef):
    """Measured on an MI355X (profiles/ppo_update_grid.txt; kernel error over the fp32 torch error per
    tensor, range over the 34 cases): 0.00-1.87, the largest at od 3 (pi_net b1 at batch 2, vf_net b2 at batch 65), and
    above 1 only at 65 rows or fewer; at 16,352 rows and more the weight gradients 0.01-0.14 and the hidden biases
    0.10-0.80 (a workgroup sums at most three tiles in fp32, the 256 partials are added in fp64).  No tensor comes
    closer to the bar than 0.38 of it; the one-element tensors are within 5.6e-8 of the reference; every statistic is
    at or below torch's error or under the floor.  All cases pass on the kernels as first merged."""
    policy, bufs, perm = _data(od)
    idx = _idx(perm, batch)
    assert idx.numel() == batch
    p64 = copy.deepcopy(policy).double()
    loss64, st64, ratio64, a64 = _loss_and_stats(p64, *(b.double() for b in bufs), idx, ent_coef)
    g64 = _grads(p64, loss64)
    # the inputs cover what they must (asserted on the reference, not on the kernel)
    assert float(_edge_distance(ratio64).min()) > EDGE
    if batch >= 257:
        for sign in (1, -1):
            s = a64 * sign > 0
            assert (s & (ratio64 > 1 + CLIP)).any() and (s & (ratio64 < 1 - CLIP)).any() and (s & ((ratio64 - 1).abs() < CLIP)).any()
    # the error an fp32 evaluation has: the largest of three row orders
    e_g, e_s = [0.0] * len(PARAM_NAMES), [0.0] * len(STAT_NAMES)
    for order in _row_orders(idx):
        loss32, st32, _, _ = _loss_and_stats(policy, *bufs, order, ent_coef)
        for k, (t32, t64) in enumerate(zip(_grads(policy, loss32), g64)):
            if float(t64.abs().max()) != 0.0:
                e_g[k] = max(e_g[k], _err(t32, t64))
        for k in range(len(STAT_NAMES)):
            if float(st64[k]) != 0.0:
                e_s[k] = max(e_s[k], _err(st32[k:k + 1], st64[k:k + 1]))
    grad, stats = _kernel_grad(policy, od, bufs, idx, ent_coef)
    kind = f"b{batch}"
    bad, off = [], 0
    for name, t64, e_t in zip(PARAM_NAMES, g64, e_g):
        x = grad[off:off + t64.numel()]
        off += t64.numel()
        if float(t64.abs().max()) == 0.0:       # (a small minibatch with every row clipped: no policy gradient at all)
            assert not bool(x.any()), name
            continue
        e_k = _err(x, t64)
        print(f"od {od} {kind} grad {name:8s} kernel {e_k:.3e} torch32 {e_t:.3e} ratio {e_k / max(e_t, 1e-30):.2f}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    assert off == grad.numel()
    for k, (name, e_t) in enumerate(zip(STAT_NAMES, e_s)):
        if float(st64[k]) == 0.0:
            assert float(stats[k]) == 0.0, name
            continue
        e_k = _err(stats[k:k + 1], st64[k:k + 1])
        print(f"od {od} {kind} stat {name:13s} kernel {e_k:.3e} torch32 {e_t:.3e}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    # every row counted once: the clip fraction is an fp64 count of integers over n, rounded once
    count64 = int(((ratio64 - 1).abs() > CLIP).sum())
    want = torch.tensor(count64 / batch, dtype=torch.float32, device=stats.device)
    assert torch.equal(stats[3], want), (float(stats[3]) * batch, count64)
    assert not bad, bad


def test_a_small_minibatch_after_a_large_one_in_the_same_workspace():
    """k_ppo_reduce reads this call's n_wg partials only: batch 70 (2 workgroups) after batch 32,869 (256) in one
    workspace gives the bits of batch 70 in a workspace that holds NaN everywhere"""
    od = 3
    policy, bufs, perm = _data(od)
    big, small = _idx(perm, 32_869), perm[100:170].contiguous()
    ws = _workspace(od)
    _kernel_grad(policy, od, bufs, big, 0.0, ws=ws)
    after = _kernel_grad(policy, od, bufs, small, 0.0, ws=ws)
    fresh = _kernel_grad(policy, od, bufs, small, 0.0, ws=_workspace(od))
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])


def test_two_calls_give_the_same_bits_at_the_full_grid():
    od = 10                                     # the largest LDS footprint
    policy, bufs, perm = _data(od)
    idx = _idx(perm, 32_869)
    a = _kernel_grad(policy, od, bufs, idx, 0.0)
    b = _kernel_grad(policy, od, bufs, idx, 0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ b747_ppo_epoch --
EPOCH_OD, EPOCH_BATCH, EPOCH_MB, N_EPOCHS, EPOCH_ENT = 5, 16_454, 3, 2, 0.0


class _State:
    """theta, Adam moments, step count, gradient, workspace and the statistics rows of one run"""

    def __init__(self, theta0, od):
        self.theta = theta0.clone()
        self.m, self.v = torch.zeros_like(theta0), torch.zeros_like(theta0)
        self.t = torch.zeros(1, dtype=torch.int64, device=theta0.device)
        self.grad = torch.full_like(theta0, float("nan"))
        self.ws = _workspace(od)
        self.stats = torch.full((N_EPOCHS * EPOCH_MB, 8), float("nan"), device=theta0.device)

    def tensors(self):
        return {"theta": self.theta, "m": self.m, "v": self.v, "t": self.t, "grad": self.grad, "stats": self.stats}


def _torch_replay(policy, bufs, perms, dtype):
    """The same minibatches in torch: _minibatch's loss, clip_grad_norm_, torch.optim.Adam(eps=1e-5)"""
    pol = copy.deepcopy(policy).to(dtype)
    opt = torch.optim.Adam(pol.parameters(), lr=LR, eps=EPS)
    views = tuple(b.to(dtype) for b in bufs)
    for perm in perms:
        for i in range(0, POOL, EPOCH_BATCH):
            loss, _, _, _ = _loss_and_stats(pol, *views, perm[i:i + EPOCH_BATCH], EPOCH_ENT)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), MAX_NORM)
            opt.step()
    return [p.detach().reshape(-1) for p in pol.flat_param_list()]


def test_epoch_call_at_the_large_shape_against_the_loop_and_fp64():
    """40,000 rows in minibatches of 16,454, 16,454 and 7,092 (515, 515 and 222 tiles: 256, 256 and 111 workgroups; the
    short one follows a full-grid one in the same workspace), two epochs"""
    from b747_rl_ctrl_amd import _lib
    L, p = _lib.lib(), lambda x: x.data_ptr()
    od = EPOCH_OD
    policy, bufs, perm = _data(od)
    dev = perm.device
    perms = (perm, torch.randperm(POOL, generator=torch.Generator().manual_seed(SEED + od + 3000)).to(dev))
    sizes = [min(EPOCH_BATCH, POOL - i) for i in range(0, POOL, EPOCH_BATCH)]
    assert sizes == [16_454, 16_454, 7_092] and len(sizes) == EPOCH_MB
    theta0 = policy.flat_params().contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    loop, call = _State(theta0, od), _State(theta0, od)
    for e in range(N_EPOCHS):
        for j, i in enumerate(range(0, POOL, EPOCH_BATCH)):
            idx = perms[e][i:i + EPOCH_BATCH].contiguous()
            _lib.check(L.b747_ppo_grad(p(loop.theta), od, *(p(b) for b in bufs), p(idx), idx.numel(), CLIP, EPOCH_ENT,
                                       VF_COEF, p(loop.ws), p(loop.grad), p(loop.stats[e * EPOCH_MB + j]), stream),
                       "b747_ppo_grad")
            _lib.check(L.b747_ppo_adam(p(loop.theta), p(loop.m), p(loop.v), p(loop.t), p(loop.grad), theta0.numel(), 1.0,
                                       MAX_NORM, LR, 0.9, 0.999, EPS, stream), "b747_ppo_adam")
        _lib.check(L.b747_ppo_epoch(p(call.theta), od, *(p(b) for b in bufs), p(perms[e]), POOL, EPOCH_BATCH, CLIP,
                                    EPOCH_ENT, VF_COEF, p(call.ws), p(call.grad), p(call.m), p(call.v), p(call.t),
                                    MAX_NORM, LR, 0.9, 0.999, EPS, p(call.stats[e * EPOCH_MB:]), stream), "b747_ppo_epoch")
    torch.cuda.synchronize()
    assert int(loop.t) == N_EPOCHS * EPOCH_MB and not torch.equal(loop.theta, theta0)
    for (name, a), b in zip(loop.tensors().items(), call.tensors().values()):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} entries differ"
    n_ws = int(L.b747_ppo_update_workspace(od))
    assert bool((loop.ws[n_ws:] == WS_GUARD).all()) and bool((call.ws[n_ws:] == WS_GUARD).all())
    ref64, ref32 = _torch_replay(policy, bufs, perms, torch.float64), _torch_replay(policy, bufs, perms, torch.float32)
    bad, off = [], 0
    for name, t32, t64 in zip(PARAM_NAMES, ref32, ref64):
        e_k, e_t = _err(call.theta[off:off + t64.numel()], t64), _err(t32, t64)
        off += t64.numel()
        print(f"od {od} epoch b{EPOCH_BATCH} theta {name:8s} kernel {e_k:.3e} torch32 {e_t:.3e} ratio {e_k / max(e_t, 1e-30):.2f}")
        if not e_k <= MARGIN * e_t + FLOOR:
            bad.append((name, e_k, e_t))
    assert off == theta0.numel()
    assert not bad, bad
