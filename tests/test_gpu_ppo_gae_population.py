"""b747_ppo_gae_population (include/b747.h, additive under ABI 15): generalized advantage estimation for
a population in one launch, env i with the gamma and gae_lambda of row i / envs_per_policy of a device table.

Yardsticks, all bit for bit (torch.equal on the int32 views of the floats, so that the NaNs an infinite reward leaves
behind an episode end compare too -- no tolerance): the torch loop of PPO.compute_gae per member on its own columns
with g = (float)gamma and gl = (float)(gamma * gae_lambda); b747_ppo_gae on a contiguous copy of each member's columns
with its scalars; and, with all rows equal, one b747_ppo_gae call on the whole batch.  Inputs are synthetic (a seeded
CPU generator).

Shapes (T, N, envs_per_policy, P): less than one chunk of 16 steps; two chunks and a partial one with the last member at
6 live lanes; two waves per member with the last member partial; T = 1 with one member."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(14, 192, 64, 3), (35, 134, 64, 3), (17, 200, 128, 2), (1, 64, 64, 1)]
COEFS = [(0.99, 0.95), (0.9, 0.6), (0.7, 1.0)]
SENTINEL, NG = -12345.0, 64


def _L():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _table(rows):
    """[P, 8] on the GPU: gamma and gae_lambda in their columns; every column the kernel must not read holds a NaN"""
    from b747_rl_ctrl_amd.ppo import HYPER_COLS, HYPER_COLUMN
    t = torch.full((len(rows), HYPER_COLS), float("nan"), dtype=torch.float64)
    for p, (g, l) in enumerate(rows):
        t[p, HYPER_COLUMN["gamma"]], t[p, HYPER_COLUMN["gae_lambda"]] = g, l
    return t.cuda()


@functools.lru_cache(maxsize=None)
def _inputs(T, N, epp, P):
    g = torch.Generator().manual_seed(7000 * T + N)
    rew, val, last_value = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g), torch.randn(N, generator=g)
    done = torch.rand(T, N, generator=g) < 0.2
    if (T, N) == CASES[0][:2]:
        # one infinite reward in member 1, late in the rollout, in an env whose episode ends before it: inf from
        # there down to the episode end, NaN (0 x inf) below it
        rew[T - 3, 70] = float("inf")
        done[4, 70] = True
    dev = torch.device("cuda")
    return tuple(x.to(dev) for x in (rew, val, done, last_value))


def _torch_gae(rew, val, done, last_value, gamma, gae_lambda):
    """PPO.compute_gae's loop with the two coefficients rounded as documented: g = (float)gamma,
    gl = (float)(gamma * gae_lambda), the fp64 product rounded once"""
    g = torch.tensor(gamma, dtype=torch.float64).float().to(rew.device)
    gl = torch.tensor(gamma * gae_lambda, dtype=torch.float64).float().to(rew.device)
    T = rew.shape[0]
    adv = torch.empty_like(rew)
    gae = torch.zeros_like(last_value)
    for t in reversed(range(T)):
        next_value = last_value if t == T - 1 else val[t + 1]
        nonterminal = (~done[t]).float()
        delta = rew[t] + g * next_value * nonterminal - val[t]
        gae = delta + gl * nonterminal * gae
        adv[t] = gae
    return adv, adv + val


@functools.lru_cache(maxsize=None)
def _reference(T, N, epp, P):
    """the torch loop per member on its columns, assembled: computed once per case, never modified"""
    rew, val, done, last_value = _inputs(T, N, epp, P)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    for p in range(P):
        sl = slice(p * epp, min((p + 1) * epp, N))
        adv[:, sl], ret[:, sl] = _torch_gae(rew[:, sl], val[:, sl], done[:, sl], last_value[sl], *COEFS[p])
    return adv, ret


def _population_call(ins, T, N, epp, P, table, adv, ret):
    _lib, L = _L()
    p = lambda x: x.data_ptr()
    rew, val, done, last_value = ins
    assert done.dtype == torch.bool and table.dtype == torch.float64 and tuple(table.shape) == (P, 8)
    _lib.check(L.b747_ppo_gae_population(p(rew), p(val), p(done), p(last_value), T, N, P, epp, p(table), p(adv), p(ret),
                                         torch.cuda.current_stream().cuda_stream), "b747_ppo_gae_population")


def _run_population(T, N, epp, P, table):
    """adv, ret [T][N] and whether the NG guard elements behind each survived"""
    ins = _inputs(T, N, epp, P)
    flat = [torch.full((T * N + NG,), SENTINEL, device=ins[0].device) for _ in range(2)]
    adv, ret = (f[:T * N].view(T, N) for f in flat)
    _population_call(ins, T, N, epp, P, table, adv, ret)
    torch.cuda.synchronize()
    return adv, ret, all(bool((f[T * N:] == SENTINEL).all()) for f in flat)


def _single_call(rew, val, done, last_value, gamma, gae_lambda):
    _lib, L = _L()
    p = lambda x: x.data_ptr()
    T, N = rew.shape
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    _lib.check(L.b747_ppo_gae(p(rew), p(val), p(done), p(last_value), T, N, gamma, gae_lambda, p(adv), p(ret),
                              torch.cuda.current_stream().cuda_stream), "b747_ppo_gae")
    torch.cuda.synchronize()
    return adv, ret


@pytest.mark.parametrize("T,N,epp,P", CASES)
def test_every_member_gets_the_bits_of_the_torch_loop_with_its_own_coefficients(T, N, epp, P):
    adv_ref, ret_ref = _reference(T, N, epp, P)
    adv, ret, guards = _run_population(T, N, epp, P, _table(COEFS[:P]))
    for p in range(P):
        sl = slice(p * epp, min((p + 1) * epp, N))
        n = adv[:, sl].numel()
        assert _same(adv[:, sl], adv_ref[:, sl]), \
            f"member {p}: adv differs in {int((_bits(adv[:, sl]) != _bits(adv_ref[:, sl])).sum())} of {n}"
        assert _same(ret[:, sl], ret_ref[:, sl]), \
            f"member {p}: ret differs in {int((_bits(ret[:, sl]) != _bits(ret_ref[:, sl])).sum())} of {n}"
    assert guards, "the elements behind adv / ret"
    if (T, N) == CASES[0][:2]:
        col = adv_ref[:, 70]
        assert bool(torch.isinf(col[T - 3])) and bool(torch.isnan(col[4])) and bool(torch.isnan(col[0]))
        keep = torch.ones(N, dtype=torch.bool, device=adv.device)
        keep[70] = False
        assert bool(torch.isfinite(adv_ref[:, keep]).all())      # the infinity stays in its env
    else:
        assert bool(torch.isfinite(adv_ref).all()) and bool(torch.isfinite(ret_ref).all())
    if P > 1:                                                    # (the members' coefficients matter)
        other = _torch_gae(*(x[..., :epp] for x in _inputs(T, N, epp, P)), *COEFS[1])[0]
        assert not _same(other, adv_ref[:, :epp])


@pytest.mark.parametrize("T,N,epp,P", CASES)
def test_every_member_gets_the_bits_of_a_single_call_on_its_own_columns(T, N, epp, P):
    rew, val, done, last_value = _inputs(T, N, epp, P)
    adv, ret, _ = _run_population(T, N, epp, P, _table(COEFS[:P]))
    for p in range(P):
        sl = slice(p * epp, min((p + 1) * epp, N))
        a, r = _single_call(rew[:, sl].contiguous(), val[:, sl].contiguous(), done[:, sl].contiguous(),
                            last_value[sl].contiguous(), *COEFS[p])
        assert _same(adv[:, sl], a) and _same(ret[:, sl], r), f"member {p}"


@pytest.mark.parametrize("T,N,epp,P", CASES)
def test_equal_rows_give_the_bits_of_one_single_call_on_the_whole_batch(T, N, epp, P):
    gamma, gae_lambda = COEFS[1]
    adv, ret, guards = _run_population(T, N, epp, P, _table([(gamma, gae_lambda)] * P))
    a, r = _single_call(*_inputs(T, N, epp, P), gamma, gae_lambda)
    assert _same(adv, a) and _same(ret, r) and guards


def test_the_inputs_and_the_table_are_left_alone():
    T, N, epp, P = CASES[1]
    ins = _inputs(T, N, epp, P)
    table = _table(COEFS[:P])
    keep = [x.clone() for x in ins] + [table.clone()]
    adv, ret = torch.empty(T, N, device=table.device), torch.empty(T, N, device=table.device)
    _population_call(ins, T, N, epp, P, table, adv, ret)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, keep)) and _same(table, keep[-1])   # (the table holds NaNs)


def test_a_captured_graph_reads_the_table_when_it_is_replayed():
    """One capture, replayed; then a table row is changed on the device and the same graph replayed again: each replay
    equals a direct call with the table as it stood (every step raises at the first error: _lib.check on the entry
    point's return value, torch on the capture, the replays and the synchronisations)"""
    T, N, epp, P = CASES[1]
    ins = _inputs(T, N, epp, P)
    before, after = _table(COEFS[:P]), _table([COEFS[0], (0.95, 0.8), COEFS[2]])
    direct = [_run_population(T, N, epp, P, t)[:2] for t in (before, after)]
    assert not _same(direct[0][0], direct[1][0])
    table = before.clone()
    adv, ret = (torch.full((T, N), SENTINEL, device=table.device) for _ in range(2))
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):          # (the capture launches nothing)
        _population_call(ins, T, N, epp, P, table, adv, ret)
    torch.cuda.synchronize()
    assert bool((adv == SENTINEL).all())
    g.replay()
    torch.cuda.synchronize()
    assert _same(adv, direct[0][0]) and _same(ret, direct[0][1])
    table[1].copy_(after[1])                     # a device copy of one row
    adv.fill_(SENTINEL)
    ret.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert _same(adv, direct[1][0]) and _same(ret, direct[1][1])
