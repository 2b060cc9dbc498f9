"""The leaves of the launch plans (csrc/b747_dispatch.h: kernel x storage type x MIX x SUB x 64 / 256 envs per workgroup)
that no other GPU test launches (profiles/refactor_dispatch/leaf_coverage.md lists every leaf with its test).  Each
case: two launches from the same start state against the generic one-wave kernel (b747_set_specialization(0)).
70 envs: two 64-env workgroups, the second ragged; 32,832 / 16,448: the first sizes with a 64-env remainder past a
threshold, where the 256-env forms start.  Tolerances are those of the module that tests the same kernel's other
leaves (tests/test_gpu_split.py, test_gpu_ppo.py, test_gpu_model.py), restated here."""
import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _env(n, x_f64=True, sample_time=None, variant="fast", seed=31):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, DisturbanceMode, ObservationType, \
        ResetRefMode, RewardType
    return BatchControllerEnv(n, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                              CtrlMode.DIRECT_CONTROL, reset_ref_mode=ResetRefMode.CONST,
                              disturbance_mode=DisturbanceMode.AERO_DISTURBANCE, tk=0.3, seed=seed, x_f64=x_f64,
                              sample_time=sample_time, variant=variant)


# tests/test_gpu_split.py _TOL.  fp64 X: ulp-level; fp32 X: both kernels round the same fp64 stage result to fp32 once
# per step, so a value next to an fp32 rounding boundary can land one fp32 ulp apart and carry forward
_TOL = {True: dict(x=1e-13, rtol=2e-6, atol=1e-7, ret_atol=1e-5, disc=1e-12),
        False: dict(x=1e-5, rtol=1e-4, atol=1e-5, ret_atol=1e-3, disc=1e-5)}

# plan_env: (api, x_f64, variant, sub, n)
_ENV_LEAVES = [("step", False, "fast", False, 70), ("step", False, "mixed", False, 70),
               ("step", False, "mixed", False, 32832),
               ("rollout", False, "fast", False, 16448), ("rollout", True, "fast", True, 16448),
               ("rollout", False, "fast", True, 16448), ("rollout", True, "mixed", False, 70),
               ("rollout", False, "mixed", False, 70), ("rollout", False, "mixed", True, 70),
               ("rollout", False, "mixed", False, 16448), ("rollout", False, "mixed", True, 16448)]


@pytest.mark.parametrize("api,x_f64,variant,sub,n", _ENV_LEAVES)
def test_split_env_kernel_leaves_equal_the_generic_one_wave_kernel(api, x_f64, variant, sub, n):
    """k_env_step_split / k_rollout_split<false> leaves.  fp64 state on FAST: the ulp-level bars; fp32 state, and MIXED
    (the flight aerodynamics in fp32: the same unit roundoff entering the state once per stage instead of once per
    step), the fp32 bars.  Integer state exactly (no episode ends in 8 steps)."""
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    tol = _TOL[x_f64 and variant == "fast"]
    K = 1 if api == "step" else 4
    envs = [_env(n, x_f64, 0.05 if sub else None, variant) for _ in range(2)]
    g = torch.Generator(device="cuda").manual_seed(17)
    prev = L.b747_set_specialization(1)
    try:
        for launch in range(2):
            acts = torch.rand(K, n, generator=g, device="cuda") * 2 - 1
            for e, spec in zip(envs, (1, 0)):
                L.b747_set_specialization(spec)
                assert e.kernel(K) == ("defc" if spec == 0 else "step_split" if api == "step" else "rollout_split")
                if api == "step":
                    e.step(acts[0])
                else:
                    e.rollout(acts)
            torch.cuda.synchronize()
            s, w = envs
            for f in ("done", "k", "episode", "ep_len", "flags", "ref", "aero_err", "state0"):
                assert torch.equal(getattr(s, f), getattr(w, f)), f"launch {launch}: {f}"
            for name, t in (("X", tol["x"]), ("disc", max(tol["x"], tol["disc"]))):
                xs, xo = getattr(s, name).double(), getattr(w, name).double()
                scale = xo.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
                err = float(((xs - xo).abs() / scale).max())
                assert err <= t, f"launch {launch}: {name} {err:.2e}"
            torch.testing.assert_close(s.obs, w.obs, rtol=tol["rtol"], atol=tol["atol"])
            torch.testing.assert_close(s.reward, w.reward, rtol=tol["rtol"], atol=tol["atol"])
            torch.testing.assert_close(s.ep_return, w.ep_return, rtol=tol["rtol"], atol=tol["ret_atol"])
    finally:
        L.b747_set_specialization(prev)


@pytest.mark.parametrize("variant", ["fast", "faithful"])
def test_one_wave_env_kernels_with_fp32_state_agree_with_each_other(variant):
    """k_env_steps<float, V, 0> (GENERIC: thrust one ulp off the DLL's default, so the constants are run-time values),
    <float, V, 2> (RECORDING) and, for FAITHFUL, <float, false, 1> (DEFC), each against k_env_steps<float, V, 1> from
    the same start state, two per-step launches of 300 envs (two workgroups, the second ragged), specialisation off.
    The same arithmetic on the same fp32 state (one ulp of thrust; FAITHFUL against FAST: ulp-level),
    each result rounded to fp32 once per step: the fp32 bars, integer state exactly."""
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    tol = _TOL[False]
    n = 300
    ref, gen, rec = (_env(n, False, None, variant) for _ in range(3))
    gen.consts.P = gen.consts.P * (1 + 2.0 ** -52)
    rec.record_signals()
    others = [("generic", gen), ("recording", rec)]
    if variant == "faithful":
        others.append(("defc", _env(n, False, None, "fast")))
    g = torch.Generator(device="cuda").manual_seed(23)
    prev = L.b747_set_specialization(0)
    try:
        assert ref.kernel() == "defc"
        for name, e in others:
            assert e.kernel() == name
        for launch in range(2):
            a = torch.rand(n, generator=g, device="cuda") * 2 - 1
            ref.step(a)
            for name, e in others:
                e.step(a)
            torch.cuda.synchronize()
            for name, e in others:
                for f in ("done", "k", "episode", "flags", "ref", "aero_err"):
                    assert torch.equal(getattr(e, f), getattr(ref, f)), f"launch {launch}: {name}: {f}"
                for field in ("X", "disc"):
                    xs, xo = getattr(e, field).double(), getattr(ref, field).double()
                    scale = xo.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
                    err = float(((xs - xo).abs() / scale).max())
                    assert err <= tol["x"], f"launch {launch}: {name}: {field} {err:.2e}"
                torch.testing.assert_close(e.obs, ref.obs, rtol=tol["rtol"], atol=tol["atol"])
                torch.testing.assert_close(e.reward, ref.reward, rtol=tol["rtol"], atol=tol["atol"])
    finally:
        L.b747_set_specialization(prev)


@pytest.mark.parametrize("sample_time", [None, 0.05])
def test_fused_ppo_rollout_mixed_small_batch_matches_the_generic_two_launch_rollout(sample_time):
    """k_rollout_split<true, double, SUB, MIX, 64>: MIXED below 32,769 envs.  128 envs (two 64-env workgroups;
    b747_ppo_rollout takes n % 64 == 0 only), two rollouts of 4 steps from the same start state against
    b747_policy_act + b747_env_step on the generic one-wave kernel (MIXED runs FAST there).  Buffers to the bars of
    tests/test_gpu_ppo.py (rtol 1e-5, atol 1e-6); the state to 1e-5 of each component's range instead of FAST's 1e-9:
    MIXED's flight aerodynamics are fp32 (unit roundoff 6e-8 into the state at every stage;
    tests/test_gpu_episode_replay.py holds 100 free steps of it to the same 1e-5)."""
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.ppo import PPO, PPOConfig
    L = _lib.lib()
    n, T = 128, 4
    e1, e2 = (_env(n, True, sample_time, "mixed", seed=3) for _ in range(2))
    p1 = PPO(e1, PPOConfig(n_steps=T, batch_size=n * T), seed=1, rollout_kernel=True)
    p2 = PPO(e2, PPOConfig(n_steps=T, batch_size=n * T), seed=1, rollout_kernel=False)
    assert p1.rollout_kernel and not p2.rollout_kernel
    prev = L.b747_set_specialization(1)
    try:
        for _ in range(2):
            p1.collect_rollouts(T)
            L.b747_set_specialization(0)
            assert e2.kernel() == "defc"
            p2.collect_rollouts(T, use_graph=True)
            L.b747_set_specialization(1)
            torch.cuda.synchronize()
            assert torch.equal(p1.done_buf, p2.done_buf)
            for a, b in ((p1.obs_buf, p2.obs_buf), (p1.act_buf, p2.act_buf), (p1.logp_buf, p2.logp_buf),
                         (p1.val_buf, p2.val_buf), (p1.rew_buf, p2.rew_buf), (e1.obs, e2.obs)):
                torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
            scale = e2.X.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
            assert float(((e1.X - e2.X).abs() / scale).max()) <= 1e-5
            assert torch.equal(e1.k, e2.k) and torch.equal(e1.episode, e2.episode)
    finally:
        L.b747_set_specialization(prev)


def _gpu_model(batch, variant):
    from b747_rl_ctrl_amd import BatchModel
    m = BatchModel(batch.n, x_f64=batch.x64, variant=variant)
    for dst, src in ((m._state0, batch.state0), (m.flags, batch.flags), (m._aero_err, batch.aero_err),
                     (m._deltaz, batch.deltaz), (m._vartheta, batch.vartheta), (m._h_zh, batch.h_zh)):
        dst.copy_(torch.from_numpy(src))
    return m


def _load_state(m, b):
    m.X.copy_(torch.from_numpy(b.X))
    m.disc.copy_(torch.from_numpy(b.disc))
    m.k.copy_(torch.from_numpy(b.k.view(np.int32)))
    m.mem.copy_(torch.from_numpy(b.mem))


def _rel(gpu, ref):
    gpu, ref = np.asarray(gpu, np.float64), np.asarray(ref, np.float64)
    scale = np.max(np.abs(ref), axis=-1, keepdims=True)
    d = np.abs(gpu - ref) / np.where(scale > 0, scale, 1.0)
    d = np.where(np.isnan(gpu) & np.isnan(ref), 0.0, d)
    return float(np.nanmax(d)) if d.size else 0.0


@pytest.mark.parametrize("variant,x64,n,k", [("fast", False, 70, 3),          # k_model_steps_split<float>, and against it
                                             ("fast", False, 16448, 3),       # k_model_step<float, FAST, 64>; <.., 256>
                                             ("faithful", True, 16448, 1),    # k_model_step<double, FAITHFUL, 256>
                                             ("faithful", False, 16448, 1)])  # k_model_step<float, FAITHFUL, 256>
def test_model_plan_leaves(variant, x64, n, k):
    """plan_model's leaves.  Two launches, each from the oracle's mid-episode state, against the one-wave kernel from the
    same state and against the oracle: the gates of tests/test_gpu_model.py (fp64 one step from identical state 1e-10,
    fp32 state 1e-5: the state rounds to fp32 once per launch, K steps of open-loop ulp differences are far below
    that; k and the Memory bits exactly)."""
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    b = O.random_batch(n, seed=41, x64=x64)
    O.oracle_initialize(b)
    O.oracle_step(b, 23)
    m, one = _gpu_model(b, variant), _gpu_model(b, variant)
    tol = 1e-10 if x64 else 1e-5
    for launch in range(2):
        _load_state(m, b)
        _load_state(one, b)
        m.step(k)
        prev = L.b747_set_specialization(0)
        try:
            one.step(k)
        finally:
            L.b747_set_specialization(prev)
        torch.cuda.synchronize()
        assert torch.equal(m.k, one.k) and torch.equal(m.mem, one.mem), launch
        assert _rel(m.X.cpu().numpy(), one.X.cpu().numpy()) <= tol, launch
        assert _rel(m.disc.cpu().numpy(), one.disc.cpu().numpy()) <= tol, launch
        O.oracle_step(b, k)
        assert np.array_equal(m.k.cpu().numpy().view(np.uint32), b.k) and np.array_equal(m.mem.cpu().numpy(), b.mem)
        for name, got, ref in (("X", m.X, b.X), ("disc", m.disc, b.disc), ("sig", m.sig, b.sig)):
            err = _rel(got.cpu().numpy(), ref)
            assert err <= tol, f"launch {launch}: {variant} x64={x64} n={n} k={k}: {name} {err:.3e}"
