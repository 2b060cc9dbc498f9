"""Batched step-response evaluation.

The reference evaluates a policy during training with `ControlTestCallback.calc_stepinfo`
(neural/callbacks.py:60-100): for each pitch reference in a list it resets ONE env at a fixed
state0 (MANUAL control, constant reference), runs the deterministic policy to tk with the
Controller's Storage recording every DLL step (core/controller.py:209-228), then computes
`calc_stepinfo` (tools/general.py:46-61) on the recorded pitch and `quality()`
(core/controller.py:334-336).  Here all test episodes run as one batch on the GPU (one env per
reference, optionally replicated) and the step-response metrics are reductions over the
recorded [T, N] pitch history.

Semantics kept from calc_stepinfo(ys, y_base, error_band=0.05, ts):
  overshoot      (max ys if y_base > 0 else min ys) - y_base) / y_base * 100; NaN if y_base == 0
  rise_time      ts[first i < T-1 with (ys[i]-ys[0])/(y_base-ys[0]) >= 1-band] - ts[0]; NaN if none
  settling_time  ts[last i outside the [1-band, 1+band] ratio band] - ts[0]; NaN if none
  static_error   |ys[-1] - y_base|
run_step_tests drives the env from Python, one recording launch per env step; run_step_tests_fused,
monte_carlo_step_tests and PPO.step_tests fly the same episodes inside ONE kernel launch with the policy in the loop and
the metrics accumulated in registers (b747_eval_episodes, include/b747.h).  population_step_tests and
pid_sweep_step_tests score many policies (one per 64-env wave) or many PID gain sets (one per env) in one such launch
(b747_eval_population).
(None in the reference -> NaN here; the reference raises ZeroDivisionError when y_base == ys[0],
which gives NaN/inf ratios here.)
"""
import math
from typing import Callable, Dict, Optional, Sequence

import torch

from .ctrl_env import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, RewardType


def stepinfo(ys: torch.Tensor, y_base: torch.Tensor, ts: torch.Tensor, error_band: float = 0.05,
             length: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """calc_stepinfo for N step responses at once: ys [T, N], y_base [N], ts [T] or [T, N]; length [N]
    (optional): env j's series is its first length[j] rows (an episode that ended early)."""
    T = ys.shape[0]
    ys = ys.to(torch.float64)
    y_base = torch.as_tensor(y_base, dtype=torch.float64, device=ys.device).expand(ys.shape[1])
    ts = torch.as_tensor(ts, dtype=torch.float64, device=ys.device)
    if ts.dim() == 1:
        ts = ts[:, None].expand_as(ys)
    L = torch.full_like(y_base, T, dtype=torch.int64) if length is None else \
        torch.as_tensor(length, device=ys.device).to(torch.int64).clamp(1, T)
    nan = torch.full_like(y_base, math.nan)
    idx = torch.arange(T, device=ys.device)[:, None].expand_as(ys)
    valid = idx < L
    peak = torch.where(y_base > 0, torch.where(valid, ys, -math.inf).max(0).values,
                       torch.where(valid, ys, math.inf).min(0).values)
    overshoot = torch.where(y_base != 0, (peak - y_base) / y_base * 100, nan)
    ratio = (ys - ys[0]) / (y_base - ys[0])
    risen = (ratio >= 1 - error_band) & (idx < L - 1)
    first = torch.where(risen, idx, T).min(0).values
    rise_time = torch.where(first < T, ts.gather(0, first.clamp(max=T - 1)[None])[0] - ts[0], nan)
    outside = ((ratio <= 1 - error_band) | (ratio >= 1 + error_band)) & valid
    last = torch.where(outside, idx, -1).max(0).values
    settling_time = torch.where(last >= 0, ts.gather(0, last.clamp(min=0)[None])[0] - ts[0], nan)
    y_end = ys.gather(0, (L - 1)[None])[0]
    return {"overshoot": overshoot, "rise_time": rise_time, "settling_time": settling_time,
            "static_error": (y_end - y_base).abs()}


def quality(itse: torch.Tensor, vartheta_ref: torch.Tensor, tk: float) -> torch.Tensor:
    """Controller.quality() (core/controller.py:334-336): exp(-60*0.1*ITSE / (tk * vref^2))."""
    return torch.exp(-60 * 0.1 * itse / (tk * vartheta_ref ** 2))


def run_step_tests(policy: Callable[[torch.Tensor], torch.Tensor], vartheta_ref: Sequence[float],
                   state0: Sequence[float] = (0, 11000, 250, 0, 0, 0), tk: float = 60.0,
                   observation_type: ObservationType = ObservationType.PID_LIKE,
                   reward_type: RewardType = RewardType.CLASSIC, ctrl_mode: Optional[CtrlMode] = CtrlMode.DIRECT_CONTROL,
                   norm_obs: bool = True, norm_act: bool = True, sample_time: Optional[float] = None,
                   replicas: int = 1, device="cuda", **env_kwargs) -> Dict[str, torch.Tensor]:
    """ControlTestCallback.calc_stepinfo for every reference at once.

    policy: deterministic actions [N] from observations [N, obs_dim] (device tensors).
    Returns per-env tensors (N = len(vartheta_ref) * replicas): settling_time, overshoot (abs, as
    the callback takes it), rise_time, static_error, quality, and the callback's means over the
    references ("mean_settling_time", "mean_overshoot", "mean_quality")."""
    refs = torch.tensor(list(vartheta_ref) * replicas, dtype=torch.float64, device=device)
    n = refs.numel()
    env = BatchControllerEnv(n, observation_type, reward_type, norm_obs, norm_act, CtrlType.MANUAL, ctrl_mode,
                             reset_ref_mode=None, tk=tk, sample_time=sample_time, auto_reset=False,
                             device=device, **env_kwargs)
    env.set_state0(torch.tensor(state0, dtype=torch.float64))
    env.set_reference(vartheta=refs)
    env.record_signals(True)
    obs = env.reset()
    steps = int(math.ceil(tk / env.sample_time - 1e-9))
    ns = int(env.cfg.n_sub)
    theta = torch.empty(steps, ns, n, dtype=torch.float64, device=device)
    ts = torch.empty(steps, ns, n, dtype=torch.float64, device=device)
    # the callback steps each episode `while not done` (neural/callbacks.py:77-80): an env that ends early
    # (use_limiter) keeps stepping here with the batch, but its series and ITSE stop at its first done
    ended = torch.zeros(n, dtype=torch.bool, device=device)
    length = torch.full((n,), steps * ns, dtype=torch.int64, device=device)
    itse = torch.zeros(n, dtype=torch.float64, device=device)
    for t in range(steps):
        obs, _, done, _ = env.step(policy(obs))
        theta[t] = torch.nan_to_num(env.signal("state_vartheta"))   # state getter, core/model.py:200
        ts[t] = env.signal("sim_time")
        live = ~ended
        itse = torch.where(live, env.signal("ITSE")[-1], itse)
        length = torch.where(live & done, (t + 1) * ns, length)
        ended = ended | done
    theta, ts = theta.reshape(steps * ns, n), ts.reshape(steps * ns, n)   # one row per DLL step
    # Storage keeps degrees for angles (core/controller.py:219-227); overshoot is unit-free
    # score against the command the dynamics ran with (b747_env_batch.ref, float64 since ABI v7)
    vref = env.ref[0].to(torch.float64)
    info = stepinfo(theta * (180 / math.pi), vref * 180 / math.pi, ts, length=length)   # (x*180)/pi like Storage
    q = quality(itse, vref, tk)
    out = {"settling_time": info["settling_time"], "overshoot": info["overshoot"].abs(),
           "rise_time": info["rise_time"], "static_error": info["static_error"], "quality": q,
           "done": ended.clone(), "length": length}
    out["mean_settling_time"] = out["settling_time"].mean()
    out["mean_overshoot"] = out["overshoot"].mean()
    out["mean_quality"] = q.mean()
    return out


# ------------------------------------------------------------------ whole episodes in one launch --

def packed_policy(policy, obs_dim: int, device) -> Optional[torch.Tensor]:
    """The packed fp32 buffer b747_eval_episodes reads (include/b747.h b747_policy_pack) for an ActorCritic, a
    fused PPO (its own `flat`, packed by sync_params) or None (no policy)."""
    if policy is None:
        return None
    flat = getattr(policy, "flat", None)
    if flat is not None:                          # PPO(fused=True)
        return flat
    if hasattr(policy, "policy") and hasattr(policy.policy, "flat_params"):   # PPO(fused=False)
        policy = policy.policy
    from . import _lib
    L = _lib.lib()
    n = int(L.b747_policy_num_params(obs_dim))
    _lib.check(min(n, 0), "b747_policy_num_params")
    buf = torch.zeros(n, dtype=torch.float32, device=device)
    with torch.no_grad():
        fp = policy.flat_params().to(device=device, dtype=torch.float32)
        buf[:fp.numel()].copy_(fp)
    _lib.check(L.b747_policy_pack(buf.data_ptr(), obs_dim, torch.cuda.current_stream(buf.device).cuda_stream),
               "b747_policy_pack")
    return buf


def _fused_out(env: BatchControllerEnv, ev: Dict[str, torch.Tensor], vref: torch.Tensor, tk: float):
    q = quality(ev["itse"], vref, tk)
    out = {"settling_time": ev["settling_time"], "overshoot": ev["overshoot"].abs(), "rise_time": ev["rise_time"],
           "static_error": ev["static_error"], "quality": q, "done": env.done.clone(),
           "length": ev["length"].to(torch.int64), "return": ev["return"]}
    out["mean_settling_time"] = out["settling_time"].mean()
    out["mean_overshoot"] = out["overshoot"].mean()
    out["mean_quality"] = q.mean()
    return out


def run_step_tests_fused(policy, vartheta_ref: Sequence[float],
                         state0: Sequence[float] = (0, 11000, 250, 0, 0, 0), tk: float = 60.0,
                         observation_type: ObservationType = ObservationType.PID_LIKE,
                         reward_type: RewardType = RewardType.CLASSIC,
                         ctrl_mode: Optional[CtrlMode] = CtrlMode.DIRECT_CONTROL, norm_obs: bool = True,
                         norm_act: bool = True, sample_time: Optional[float] = None, replicas: int = 1, device="cuda",
                         ctrl_type: CtrlType = CtrlType.MANUAL, action=None, **env_kwargs) -> Dict[str, torch.Tensor]:
    """run_step_tests with every episode flown inside ONE kernel launch (BatchControllerEnv.eval_episodes): the
    deterministic policy runs in the kernel's step loop and the step-response metrics accumulate in registers, so
    neither the per-step host round trips nor the [steps, n_sub, N] history of run_step_tests exist.

    policy: an ActorCritic, a PPO (its packed `flat` buffer) or None -- then `action` [N] or scalar (default 0) is
    held for the whole episode; with ctrl_type AUTO / FULL_AUTO the SS PID flies and the action is ignored (the
    PID baseline of agent_test.pid_baseline_env).  Same series (theta * (180 / pi) against vref * 180 / pi) and the
    same keys as run_step_tests, plus "return" (the episode return)."""
    refs = torch.tensor(list(vartheta_ref) * replicas, dtype=torch.float64, device=device)
    n = refs.numel()
    env = BatchControllerEnv(n, observation_type, reward_type, norm_obs, norm_act, ctrl_type, ctrl_mode,
                             reset_ref_mode=None, tk=tk, sample_time=sample_time, auto_reset=False,
                             device=device, **env_kwargs)
    env.set_state0(torch.tensor(state0, dtype=torch.float64))
    env.set_reference(vartheta=refs)
    env.reset()
    steps = int(math.ceil(tk / env.sample_time - 1e-9))
    vref = env.ref[0].to(torch.float64)
    ev = env.eval_episodes(steps, packed_policy(policy, env.obs_dim, env.device), "state_vartheta",
                           scale=180 / math.pi, y_base=vref * 180 / math.pi, action=action)
    out = _fused_out(env, ev, vref, tk)
    out["env"] = env
    return out


# ------------------------------------------------- populations: policies and PID gain sets in one launch --

def pack_policies(policies, obs_dim: int, device) -> torch.Tensor:
    """[P, stride] packed fp32 policies for BatchControllerEnv.eval_population, filled by ONE b747_policy_pack_batch
    launch: row p is what packed_policy gives for policy p (stride = b747_policy_num_params, a multiple of 4).
    policies: a sequence of ActorCritic / PPO, or a [P, n] tensor of ActorCritic.flat_params() rows."""
    from . import _lib
    L = _lib.lib()
    stride = int(L.b747_policy_num_params(obs_dim))
    _lib.check(min(stride, 0), "b747_policy_num_params")
    if torch.is_tensor(policies):
        rows = policies.detach()
        assert rows.dim() == 2, "policies: [P, n] flat_params rows"
    else:
        flats = []
        for p in policies:
            net = p.policy if hasattr(p, "policy") and hasattr(p.policy, "flat_params") else p
            flats.append(net.flat_params().detach())
        rows = torch.stack(flats)
    assert 1 <= rows.shape[1] <= stride, "policies: flat_params rows of this obs_dim"
    buf = torch.zeros(rows.shape[0], stride, dtype=torch.float32, device=device)
    buf[:, :rows.shape[1]].copy_(rows.to(device=device, dtype=torch.float32))
    _lib.check(L.b747_policy_pack_batch(buf.data_ptr(), obs_dim, buf.shape[0], stride,
                                        torch.cuda.current_stream(buf.device).cuda_stream), "b747_policy_pack_batch")
    return buf


def _population_out(env, ev, vref, tk, groups: int, group: int, keep: int) -> Dict[str, torch.Tensor]:
    """_fused_out as [groups, keep] (the first `keep` envs of every `group`-env group; the last group may be
    partial), the callback's means per group and the group with the best mean quality"""
    flat = _fused_out(env, ev, vref, tk)
    idx = (torch.arange(groups, device=env.device)[:, None] * group + torch.arange(keep, device=env.device)[None])
    out = {k: v[idx] for k, v in flat.items() if torch.is_tensor(v) and v.dim() == 1}
    out["mean_settling_time"] = out["settling_time"].mean(1)
    out["mean_overshoot"] = out["overshoot"].mean(1)
    out["mean_quality"] = out["quality"].mean(1)
    out["best"] = out["mean_quality"].argmax()
    return out


def population_step_tests(policies, vartheta_ref: Sequence[float],
                          state0: Sequence[float] = (0, 11000, 250, 0, 0, 0), tk: float = 60.0,
                          observation_type: ObservationType = ObservationType.PID_LIKE,
                          reward_type: RewardType = RewardType.CLASSIC,
                          ctrl_mode: Optional[CtrlMode] = CtrlMode.DIRECT_CONTROL, norm_obs: bool = True,
                          norm_act: bool = True, sample_time: Optional[float] = None, device="cuda",
                          ctrl_type: CtrlType = CtrlType.MANUAL, **env_kwargs) -> Dict[str, torch.Tensor]:
    """run_step_tests_fused for P policies in ONE launch: policy p flies the 64-env group p (the references repeated
    to fill it; only its first len(vartheta_ref) envs are reported).  policies: what pack_policies takes.  Returns every metric of run_step_tests_fused as [P, R], the callback's
    "mean_quality" / "mean_overshoot" / "mean_settling_time" as [P], and "best" (argmax of the mean quality)."""
    R = len(vartheta_ref)
    assert 1 <= R <= 64, "one 64-env group per policy"
    dev = _lib_device(device)
    obs_dim = {ObservationType.PID_LIKE: 3, ObservationType.SPEED_MODE: 5}[observation_type]
    packed = pack_policies(policies, obs_dim, dev)
    P = int(packed.shape[0])
    n = (P - 1) * 64 + R                  # the last group needs its reported envs only
    refs = torch.tensor((list(vartheta_ref) * 64)[:64] * P, dtype=torch.float64, device=dev)[:n]
    env = BatchControllerEnv(n, observation_type, reward_type, norm_obs, norm_act, ctrl_type, ctrl_mode,
                             reset_ref_mode=None, tk=tk, sample_time=sample_time, auto_reset=False,
                             device=dev, **env_kwargs)
    env.set_state0(torch.tensor(state0, dtype=torch.float64))
    env.set_reference(vartheta=refs)
    env.reset()
    steps = int(math.ceil(tk / env.sample_time - 1e-9))
    vref = env.ref[0].to(torch.float64)
    ev = env.eval_population(steps, packed, 64, signal="state_vartheta", scale=180 / math.pi,
                             y_base=vref * 180 / math.pi)
    out = _population_out(env, ev, vref, tk, P, 64, R)
    out["env"] = env
    return out


def pid_sweep_step_tests(gains, vartheta_ref: Sequence[float], loop: str = "SS", policy=None,
                         state0: Sequence[float] = (0, 11000, 250, 0, 0, 0), tk: float = 60.0,
                         observation_type: ObservationType = ObservationType.PID_LIKE,
                         reward_type: RewardType = RewardType.CLASSIC, ctrl_mode: Optional[CtrlMode] = None,
                         norm_obs: bool = True, norm_act: bool = True, sample_time: Optional[float] = None,
                         device="cuda", **env_kwargs) -> Dict[str, torch.Tensor]:
    """G sets of PID gains (gains [G, 4]) against R references in ONE launch of G * R envs: env g * R + r flies gain
    set g against reference r.  loop "SS": the pitch-stabilisation PID's gains, vartheta_ref are pitch commands and
    the pitch series is scored; "CS": the altitude-hold PID's gains, vartheta_ref are ALTITUDE commands and the
    altitude series is scored against them (as agent_test.controller_test does).  policy None: the PID baseline
    (AUTO for "SS", FULL_AUTO for "CS": agent_test.pid_baseline_env; sample_time defaults to dt).  With a policy
    (loop "SS") ctrl_mode must be one of the ADD modes: the policy, one for every env, flies on top of the swept SS
    PID.  Returns every metric as [G, R], the means as [G] and "best".  For "SS", "quality" is Controller.quality()
    and best = argmax of its mean; for "CS" that formula needs the CS PID's last pitch command, which the kernel
    does not return: "quality" is absent there and best = argmin of the mean ITSE it is built on."""
    assert loop in ("SS", "CS")
    dev = _lib_device(device)
    g = torch.as_tensor(gains, dtype=torch.float64)
    assert g.dim() == 2 and g.shape[1] == 4, "gains: [G, 4]"
    G, R = int(g.shape[0]), len(vartheta_ref)
    n = G * R
    if policy is None:
        ctrl_type = CtrlType.AUTO if loop == "SS" else CtrlType.FULL_AUTO
    else:
        assert loop == "SS" and ctrl_mode in (CtrlMode.ADD_DIRECT_CONTROL, CtrlMode.ADD_PROC_CONTROL), \
            "a policy flies on top of the swept SS PID in the ADD control modes only"
        ctrl_type = CtrlType.MANUAL
    refs = torch.tensor(list(vartheta_ref) * G, dtype=torch.float64, device=dev)
    env = BatchControllerEnv(n, observation_type, reward_type, norm_obs, norm_act, ctrl_type, ctrl_mode,
                             reset_ref_mode=None, tk=tk, sample_time=sample_time, auto_reset=False,
                             device=dev, **env_kwargs)
    env.set_state0(torch.tensor(state0, dtype=torch.float64))
    if loop == "SS":
        env.set_reference(vartheta=refs)
    else:
        env.set_reference(h=refs)
    env.reset()
    steps = int(math.ceil(tk / env.sample_time - 1e-9))
    per_env = g.to(dev).repeat_interleave(R, 0)               # [G * R, 4]
    params, epp = None, 64
    if policy is not None:                                      # one policy for the whole batch: one group
        params = packed_policy(policy, env.obs_dim, env.device)[None]
        epp = (n + 63) // 64 * 64
    kw = dict(signal="state_vartheta", scale=180 / math.pi, y_base=refs * 180 / math.pi) if loop == "SS" else \
        dict(signal="state_y", scale=1.0, y_base=refs)
    ev = env.eval_population(steps, params, epp, pid_ss=per_env if loop == "SS" else None,
                             pid_cs=per_env if loop == "CS" else None, **kw)
    out = _population_out(env, ev, refs, tk, G, R, R)
    out["itse"] = ev["itse"].reshape(G, R)
    if loop == "CS":
        for k in ("quality", "mean_quality"):
            del out[k]
        out["best"] = out["itse"].mean(1).argmin()
    out["env"] = env
    return out


def _lib_device(device):
    from . import _lib
    return _lib.resolve_device(device)


def monte_carlo_step_tests(policy, n: int, seed: int = 0, tk: float = 20.0,
                           observation_type: ObservationType = ObservationType.PID_LIKE,
                           reward_type: RewardType = RewardType.CLASSIC,
                           ctrl_mode: Optional[CtrlMode] = CtrlMode.DIRECT_CONTROL, norm_obs: bool = True,
                           norm_act: bool = True, sample_time: Optional[float] = 0.05, env_offset: int = 0,
                           quantiles: Sequence[float] = (0.05, 0.5, 0.95), device="cuda",
                           **env_kwargs) -> Dict[str, torch.Tensor]:
    """A Monte-Carlo robustness test of one controller: n envs with the reference's random resets (CONST pitch
    references, random initial states, drawn aerodynamic errors: core/controller.py:134-201), one step-response
    episode each, all in one launch.  The draws are Philox streams keyed by (seed, env_offset + i), so env i's
    result does not depend on how the n envs are split into batches (shard with env_offset).

    Returns the per-env metrics of run_step_tests_fused plus "vartheta_ref" [n], and for each metric m:
    "<m>_quantiles" [len(quantiles)] over the envs where it is defined and "<m>_nan_share" (rise / settling time
    are NaN for an env that never rises / never leaves the band)."""
    from .ctrl_env import DisturbanceMode, ResetRefMode
    env = BatchControllerEnv(n, observation_type, reward_type, norm_obs, norm_act, CtrlType.MANUAL, ctrl_mode,
                             reset_ref_mode=ResetRefMode.CONST, disturbance_mode=DisturbanceMode.AERO_DISTURBANCE,
                             tk=tk, sample_time=sample_time, auto_reset=False, seed=seed, env_offset=env_offset,
                             device=device, **env_kwargs)      # (the constructor resets once: the draws)
    steps = int(math.ceil(tk / env.sample_time - 1e-9))
    vref = env.ref[0].to(torch.float64).clone()
    ev = env.eval_episodes(steps, packed_policy(policy, env.obs_dim, env.device), "state_vartheta",
                           scale=180 / math.pi, y_base=vref * 180 / math.pi)
    out = _fused_out(env, ev, vref, tk)
    out["vartheta_ref"] = vref
    qs = torch.tensor(list(quantiles), dtype=torch.float64, device=env.device)
    for m in ("overshoot", "rise_time", "settling_time", "static_error", "quality"):
        v = out[m]
        nan = torch.isnan(v)
        out[m + "_nan_share"] = nan.double().mean()
        out[m + "_quantiles"] = torch.nanquantile(v, qs) if not bool(nan.all()) else torch.full_like(qs, math.nan)
    return out
