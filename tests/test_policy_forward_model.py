"""The policy forward pass of csrc/b747_policy.h against float64, on the CPU: the policies, observation sets, reference,
yardstick and bar that tests/test_gpu_policy_forward_f64.py holds the kernels to, and a restatement of the kernels'
arithmetic in numpy that shows the bar is one the design meets and a broken design misses.  No GPU, no library.

Reference: ActorCritic(od).double() on the CPU.  Yardstick: the same module in fp32 on the CPU.  err(x) = max over rows
|x - x64|.  Bar, for mean and value separately, per case:

    err <= 16 err(torch32) + 2^-22 max(1, max |x64|)

16 = 2^2 for the two significand bits the f16 hi/lo split gives up against fp32 (three products keep ~22 bits), times
the MARGIN = 4 of tests/test_gpu_ppo_update.py for summation order; the floor is one unit of the design precision at the
output's scale.  Log-probability, per row, first order in the error of the mean:

    |logp - logp64(a; mean64, sigma)| <= (|z| / sigma) (B_mean + 2^-24 |a|) + 2^-22 max(1, |logp64|)

with a the stored action, B_mean the case's bar for the mean and |z| = sqrt(max(0, -2 (logp + log_std + c))) in float64.

Policies: one seeded ActorCritic per obs_dim, + 0.05 randn on every parameter, then every tensor except log_std times
g in {1, 3, 10}: g = 1 is the initialisation scale every other test runs at, 3 and 10 what training moves towards
(saturated tanh units).  Observation sets (1,094 rows = 4 x 256 + 64 + 6 unless a kernel needs another count): randn x
s for s in {1e-3, 1, 10}; "mixed", each row at its own scale 10^U(-4, 2); each with a tail of 36 edge rows that carry
one edge value in one component: 0, +-6e-8, +-6.1e-5 and +-0.125 (the f16 subnormal threshold, and the threshold below
which the lo half of the split is subnormal), +-65504, 65520, 7e4 and -3e38 (the clamp of the matrix-core layer 1).

The model, from the comments of b747_policy.h and sharing no code with it: hi = f16(x), lo = f16(f32(x - hi)); products
hi hi + hi lo + lo hi summed exactly and rounded to f32 once per layer; the derived parameters s W1, s b1,
s (b2 + W2 1), -2 s W2, -2 w, b + sum w in f32 (s = 2 / ln 2); layer 1 for obs_dim <= 4 as such a split product with the
observations clamped to +-65504, for larger obs_dim an f32 fma chain; sig(u) = 1 / (2^u + 1) with 2^u, the sum and the
reciprocal each correctly rounded to f32.  It is the design at its best: what the kernels lose beyond it (hardware
exp2 / rcp at 1 ulp, the matrix cores' own accumulation) is theirs to keep inside the same bar."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

SEED = 29
GS = (1, 3, 10)
SETS = ("s1e-3", "s1", "s10", "mixed")
N_ROWS = 1094
EDGE = (0.0, 6e-8, -6e-8, 6.1e-5, -6.1e-5, 0.125, -0.125, 65504.0, -65504.0, 65520.0, 7e4, -3e38)
N_EDGE = 3 * len(EDGE)
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
F16_MIN_NORMAL = 2.0 ** -14


# ---------------------------------------------------------------- policies, observations, reference, bar

@functools.lru_cache(maxsize=None)
def _policy(od, g):
    from b747_rl_ctrl_amd.ppo import ActorCritic
    gen = torch.Generator().manual_seed(SEED + od)
    torch.manual_seed(SEED + od)
    net = ActorCritic(od)
    with torch.no_grad():
        for prm in net.flat_param_list():
            prm.add_(0.05 * torch.randn(prm.shape, generator=gen))
        for prm in net.flat_param_list()[:-1]:
            prm.mul_(float(g))
        net.log_std.fill_(0.0)
    return net


def policy(od, g, log_std=0.0):
    """a fresh fp32 CPU copy of the (od, g) policy with the given log_std"""
    net = copy.deepcopy(_policy(od, g))
    with torch.no_grad():
        net.log_std.fill_(float(log_std))
    return net


@functools.lru_cache(maxsize=None)
def observations(od, name, n=N_ROWS):
    """[n, od] fp32 on the CPU; the last N_EDGE rows carry the edge values"""
    gen = torch.Generator().manual_seed(1000 * SEED + 10 * od + SETS.index(name))
    x = torch.randn(n, od, generator=gen)
    if name == "mixed":
        x = x * 10.0 ** (6.0 * torch.rand(n, 1, generator=gen) - 4.0)
    else:
        x = x * float(name[1:])
    for r in range(N_EDGE):
        x[n - N_EDGE + r, r % od] = EDGE[r % len(EDGE)]
    assert bool(torch.isfinite(x).all())
    return x


def err(x, x64):
    return float((x.double().reshape(-1) - x64.reshape(-1)).abs().max())


def bar(err32, x64):
    return 16.0 * err32 + 2.0 ** -22 * max(1.0, float(x64.abs().max()))


def forward64(net, obs):
    """(mean64 [n], value64 [n]) of an fp32 policy in float64 on the CPU"""
    with torch.no_grad():
        mean, value = copy.deepcopy(net).double()(obs.double().cpu())
    return mean.reshape(-1), value.reshape(-1)


def yardstick(net, obs):
    """mean64, value64, err(torch32) and the bar of both outputs for an fp32 policy on fp32 observations"""
    obs = obs.detach().cpu().float()
    mean64, val64 = forward64(net, obs)
    assert bool(torch.isfinite(mean64).all() and torch.isfinite(val64).all()), "the float64 reference is finite"
    with torch.no_grad():
        mean32, val32 = copy.deepcopy(net).float()(obs)
    e_mean, e_val = err(mean32, mean64), err(val32, val64)
    return {"mean64": mean64, "val64": val64, "err32_mean": e_mean, "err32_val": e_val,
            "bar_mean": bar(e_mean, mean64), "bar_val": bar(e_val, val64)}


@functools.lru_cache(maxsize=None)
def reference(od, g, name, n=N_ROWS):
    return yardstick(_policy(od, g), observations(od, name, n))


def logp_check(logp, act, mean64, log_std, bar_mean):
    """(|logp - logp64(act)|, its bound) per row in float64; logp, act: the kernel's stored fp32 values"""
    logp, act = logp.detach().double().cpu().reshape(-1), act.detach().double().cpu().reshape(-1)
    log_std = float(torch.tensor(log_std, dtype=torch.float32))      # the fp32 parameter the kernel reads
    sigma = math.exp(log_std)
    logp64 = -(act - mean64) ** 2 / (2 * sigma * sigma) - log_std - LOG_SQRT_2PI
    z = (-2.0 * (logp + log_std + LOG_SQRT_2PI)).clamp_min(0.0).sqrt()
    bound = z / sigma * (bar_mean + 2.0 ** -24 * act.abs()) + 2.0 ** -22 * logp64.abs().clamp_min(1.0)
    return (logp - logp64).abs(), bound


def saturated_units(net, obs, level=0.999):
    """[n] the number of hidden units (both layers, both nets) with |tanh| > level in the float64 reference"""
    net64, x = copy.deepcopy(net).double(), obs.double()
    count = torch.zeros(obs.shape[0], dtype=torch.int64)
    with torch.no_grad():
        for seq in (net64.pi_net, net64.vf_net):
            h = x
            for layer in seq:
                h = layer(h)
                if isinstance(layer, torch.nn.Tanh):
                    count += (h.abs() > level).sum(1)
    return count


# ---------------------------------------------------------------- the arithmetic of b747_policy.h, restated

S = np.float32(2.0 / math.log(2.0))


def _f16(x, flush):
    h = np.asarray(x, dtype=np.float32).astype(np.float16)
    if flush:
        h = np.where(np.abs(h.astype(np.float32)) < F16_MIN_NORMAL, np.float16(0.0), h)
    return h


def _split(x, flush):
    """x (f32) = hi + lo, both f16, returned as float64 arrays"""
    x = np.asarray(x, dtype=np.float32)
    hi = _f16(x, flush)
    lo = _f16(x - hi.astype(np.float32), flush)          # x - hi is exact in f32
    return hi.astype(np.float64), lo.astype(np.float64)


def _split_matmul(a, x, lo_hi, flush):
    """[n, out]: sum_k of the split products of a [out, k] (the weights' side) and x [n, k], exact"""
    ah, al = _split(a, flush)
    xh, xl = _split(x, flush)
    out = xh @ ah.T + xl @ ah.T
    if lo_hi:
        out = out + xh @ al.T
    return out


def _sig(u):
    with np.errstate(over="ignore"):
        e = np.exp2(u.astype(np.float64)).astype(np.float32)
        return (np.float64(1.0) / (e + np.float32(1.0)).astype(np.float64)).astype(np.float32)


def _sum32(first, terms):
    """first + terms[..., 0] + terms[..., 1] + ... one f32 addition at a time"""
    a = np.asarray(first, dtype=np.float32).copy()
    for k in range(terms.shape[-1]):
        a = (a + terms[..., k].astype(np.float32)).astype(np.float32)
    return a


def model_forward(net, obs, lo_hi=True, flush=False):
    """(mean, value) as float32 arrays [n] by the arithmetic of the header (module docstring); lo_hi=False drops the
    lo hi product of both matrix-core layers, flush=True flushes f16 subnormals to zero"""
    od = obs.shape[1]
    f32 = lambda t: t.detach().numpy().astype(np.float32)
    x = f32(obs)
    outs = []
    for seq, head in ((net.pi_net, net.action_net), (net.vf_net, net.value_net)):
        w1, b1, w2, b2 = f32(seq[0].weight), f32(seq[0].bias), f32(seq[2].weight), f32(seq[2].bias)
        w, b = f32(head.weight).reshape(-1), f32(head.bias).reshape(-1)
        if od <= 4:
            # layer 1 on the matrix cores: the observation clamped to the f16 range, the bias in K as hi(s b1) +
            # lo(s b1) against 1
            bh, bl = _split(S * b1, flush)
            xc = np.clip(x, np.float32(-65504.0), np.float32(65504.0))
            u1 = (_split_matmul(S * w1, xc, lo_hi, flush) + (bh + bl)).astype(np.float32)
        else:
            # layer 1 on the VALU: an f32 fma chain from s b1 over the od inputs (no split, no clamp)
            with np.errstate(over="ignore", invalid="ignore"):
                u1 = np.broadcast_to(S * b1, (x.shape[0], b1.shape[0])).astype(np.float32)
                for k in range(od):
                    u1 = ((S * w1[:, k]).astype(np.float64)[None, :] * x[:, k].astype(np.float64)[:, None]
                          + u1.astype(np.float64)).astype(np.float32)
        r1 = _sig(u1)
        # layer 2: s z2 = s (b2 + W2 1) + (-2 s W2) r1
        acc0 = S * _sum32(b2, w2)
        u2 = (acc0.astype(np.float64) + _split_matmul(np.float32(-2.0) * S * w2, r1, lo_hi, flush)).astype(np.float32)
        r2 = _sig(u2)
        # head: (b + sum w) + sum (-2 w) sig(s z2)
        c = _sum32(b[0], w)
        hw = (np.float32(-2.0) * w).astype(np.float64)
        outs.append((r2.astype(np.float64) @ hw).astype(np.float32) + c)
    return outs[0], outs[1]


def _model_errs(g, name, **kw):
    ref = reference(3, g, name)
    mean, value = model_forward(_policy(3, g), observations(3, name), **kw)
    return ref, err(torch.from_numpy(mean), ref["mean64"]), err(torch.from_numpy(value), ref["val64"])


CASES = [(g, name) for g in GS for name in SETS]


@pytest.mark.parametrize("g,name", CASES)
def test_the_design_meets_the_bar(g, name):
    ref, e_mean, e_val = _model_errs(g, name)
    print(f"model od 3 g {g} {name}: mean {e_mean:.3e} torch32 {ref['err32_mean']:.3e} bar {ref['bar_mean']:.3e} | "
          f"value {e_val:.3e} torch32 {ref['err32_val']:.3e} bar {ref['bar_val']:.3e}")
    assert e_mean <= ref["bar_mean"], (e_mean, ref["err32_mean"], ref["bar_mean"])
    assert e_val <= ref["bar_val"], (e_val, ref["err32_val"], ref["bar_val"])


@pytest.mark.parametrize("broken", [{"lo_hi": False}, {"flush": True}], ids=["no_lo_hi", "subnormals_flushed"])
@pytest.mark.parametrize("g,name", CASES)
def test_a_broken_split_misses_the_bar(g, name, broken):
    """the bar has teeth: without the lo hi product, or with f16 subnormals flushed, the same model is outside it"""
    ref, e_mean, e_val = _model_errs(g, name, **broken)
    print(f"model od 3 g {g} {name} {broken}: mean {e_mean / ref['bar_mean']:.1f} x bar, value {e_val / ref['bar_val']:.1f} x bar")
    assert e_mean > ref["bar_mean"] and e_val > ref["bar_val"], (e_mean, ref["bar_mean"], e_val, ref["bar_val"])


@pytest.mark.parametrize("od", [3, 5, 7, 8, 10])
def test_the_cases_are_what_they_claim(od):
    for name in SETS:
        x = observations(od, name).abs()
        assert bool(((x > 0) & (x < 0.125)).any()) and bool((x > 1).any()), name
        assert int((x > 65504).sum()) == 9 and int((x == 0).sum()) >= 3, name
        for g in GS:
            ref = reference(od, g, name)
            assert ref["err32_mean"] > 0 and ref["err32_val"] > 0, (g, name)
        assert bool((saturated_units(_policy(od, 10), observations(od, name)) > 0).any()), name
    # g = 1: rows with no saturated unit at all, wherever the observations are not large themselves
    for name in ("s1e-3", "s1", "mixed"):
        assert bool((saturated_units(_policy(od, 1), observations(od, name)) == 0).any()), name


def test_the_model_is_the_torch_policy():
    """guards the restatement itself: at g = 1 on ordinary observations it is the float64 policy within 1e-5"""
    ref, e_mean, e_val = _model_errs(1, "s1")
    assert e_mean < 1e-5 and e_val < 1e-5
