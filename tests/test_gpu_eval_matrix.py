"""b747_eval_episodes (k_eval_episodes, BatchControllerEnv.eval_episodes) at state level, over the configuration matrix
include/b747.h claims for it ("every configuration b747_env_step covers, run-time constants, FAST or FAITHFUL"; every
buffer "as a step loop would leave" it), against references that are not the episode kernel:

  1. test_state_parity_with_the_step_loop -- 13 configurations x FAITHFUL / FAST, 70 envs (two waves, the second with 6
     live lanes), params == NULL with a per-env held action.  Env A flies one eval_episodes launch, env B a host loop
     of step() (b747_env_step) with every buffer's column snapshotted at the env's first done.  Compared: X, disc, k,
     mem, deltaz, upid, tp, h_zh, ep_return, ep_final_return, ep_final_len, ep_stats, obs, reward, done, terminal_obs,
     and the eval rows length == k, return == ep_return (row 1 once more with signal recording on in B: itse == the
     ITSE signal of B's last DLL step).
     FAITHFUL: both kernels run the same env_step_lane without FMA contraction -- every buffer bit for bit (NaN == NaN).
     Found bit-equal in all 13 rows on an MI355X: the DEFC step kernel's literal constants against the episode kernel's
     run-time constants change no rounding.
     FAST: integer / flag buffers exact; float64 buffers against the CPU oracle (tests/oracle_lib.EnvOracle, fed the
     draws read back from the device, with env.consts written into its models): the step loop's deviation from the
     oracle is measured per component as a share of the component's largest magnitude over the batch, and the episode
     kernel may deviate at most twice as much, never held below 1e-13 (the floor of
     test_gpu_env.test_specialised_kernel_equals_generic_kernel); a slot the configuration does not keep (deltaz
     outside ANG_VEL, ...) has no oracle value and must equal the step loop's bit for bit.  float32 obs / reward /
     terminal_obs against the oracle at the project's rtol 2e-6, atol 1e-7.
  2. test_eval_rows_against_the_cpu_restatement -- 8 envs, oracle/ref_env.py with its per-DLL-step record hook and
     calc_stepinfo: the four step-info rows on three different scored series (sig_row, scale, error_band varied, a
     y_base of 0 and negative ones), the itse row, the length and the return row, for MANUAL / DIRECT and AUTO.
  3. the launch's own edges, FAITHFUL and exact: a launch shorter than the episode and a second call; the clip of the
     policy path against the held-action path (obs_dim 3 and 5, [-1, 1] and [-0.5, 0.25]); sentinel columns around
     y_base and eval_out in every 70-env launch (lanes past n step a copy of env n - 1 and must store nothing).

Measured on an MI355X (FAST; the test prints the table; deviation from the oracle as a share of the component's largest
magnitude, maximum over the components of X and disc and over the 70 envs).  One figure where the step loop's and the
episode kernel's agree to the two digits printed (every row but 5), else step loop / episode kernel:

  row   X                  disc     slot                 ep_return (float32-valued)
   1    4.3e-16            3.2e-14                       1.3e-09
   2    4.1e-16            1.7e-14                       3.1e-08
   3    1.9e-14            4.4e-14  upid   4.2e-14       1.0e-07
   4    7.6e-15            7.5e-14  upid   4.8e-14       1.3e-07
   5    4.6e-16 / 4.1e-16  2.7e-14  deltaz 9.4e-17 / 0   6.5e-08
   6    3.6e-16            7.9e-15  tp     0             0
   7    8.2e-15            5.3e-14                       0
   8    1.6e-14            1.1e-13  h_zh   0             7.0e-08
   9    7.4e-16            1.8e-14  h_zh   0             7.0e-08
  10    5.1e-16            2.3e-14                       7.0e-08
  11    4.7e-16            5.0e-14  deltaz 0             6.9e-08
  12    3.2e-16            1.9e-14  h_zh   0             1.4e-07
  13    5.1e-16            1.8e-14                       5.2e-10
  ITSE signal at the last DLL step (row 1, step loop recording): 2.9e-16

Before the kernel wrote them, rows 1-13 failed on obs (with params == NULL it kept the reset's zeros; measured on the
kernel as it was) and terminal_obs was never written (it is compared after obs).
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O
from stepinfo_ref import calc_stepinfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_env as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 70
RTOL, ATOL = 2e-6, 1e-7              # float32 obs / reward against the oracle (tests/test_gpu_env.py)
FLOOR = 1e-13                         # of a component's magnitude (test_specialised_kernel_equals_generic_kernel)
SENT = -1.2345678e300                 # guard value around y_base / eval_out
BUFS = ("X", "disc", "k", "mem", "deltaz", "upid", "tp", "h_zh", "ep_return", "ep_final_return", "ep_final_len",
        "ep_stats", "obs", "reward", "done", "terminal_obs")
ROW_MAJOR = ("obs", "terminal_obs")   # [N, obs_dim]; every other buffer has the env index last
EXACT = ("k", "mem", "done", "ep_final_len")


def _rows():
    from b747_rl_ctrl_amd import (CtrlMode as M, CtrlType as C, DisturbanceMode as D, ObservationType as Ob,
                                  ResetRefMode as Rm, RewardType as Rw)
    base = dict(obs=Ob.PID_LIKE, rew=Rw.CLASSIC, ct=C.MANUAL, cm=M.DIRECT_CONTROL)
    semi = dict(obs=Ob.SPEED_MODE, rew=Rw.CLASSIC, ct=C.SEMI_MANUAL, cm=M.DIRECT_CONTROL)
    return {
        1: dict(base),
        2: dict(base, sample_time=None, tk=0.5),
        # preset (rows 3, 5, 6): the slots a reset zeroes (upid, deltaz) or leaves alone (tp: never reset, as in the
        # reference) start from drawn values, so that a kernel which does not load them is seen in a first launch
        3: dict(obs=Ob.SPEED_MODE, rew=Rw.PID_LIKE, ct=C.MANUAL, cm=M.ADD_PROC_CONTROL, preset=True),
        4: dict(obs=Ob.PID_AERO, rew=Rw.QUALITY, ct=C.MANUAL, cm=M.ADD_DIRECT_CONTROL, reset=Rm.CONST,
                dist=D.AERO_DISTURBANCE),
        5: dict(obs=Ob.PID_SPEED_AERO, rew=Rw.MINIMAL, ct=C.MANUAL, cm=M.ANG_VEL_CONTROL, norm=False,
                preset=True),
        6: dict(obs=Ob.MODEL_STATE, rew=Rw.TF_REFERENCE, ct=C.MANUAL, cm=M.DIRECT_CONTROL, reset=Rm.OSCILLATING,
                preset=True),
        7: dict(obs=Ob.MODEL_STATE, rew=Rw.PID_LIKE, ct=C.AUTO, cm=None),
        8: dict(base, ct=C.FULL_AUTO, cm=None),
        9: dict(semi),
        10: dict(base, reset=Rm.HYBRID),
        # ANG_VEL integrates a * action_max * sample_time per env step: with action_max 5 deg (below the 17 deg
        # clip) an env with a > 0.5 crosses deltaz > action_max at step floor(20 / a) + 1 <= 40, one with a small
        # action runs to tk unless the pitch limiter ends it: the actions are scaled by 1, 0.5, 0.05 in turn
        11: dict(base, cm=M.ANG_VEL_CONTROL, use_limiter=True, tk=2.0, action_max=5 * math.pi / 180,
                 act_scale=(1.0, 0.5, 0.05)),
        12: dict(semi, consts=True),
        13: dict(obs=Ob.PID_AERO, rew=Rw.CLASSIC, ct=C.MANUAL, cm=M.DIRECT_CONTROL, dist=D.AERO_DISTURBANCE,
                 aero_err=[-0.2, 0.15, -0.05, 0.1, 0.3]),
    }


def _mk(r, variant, n=N, seed=5):
    from b747_rl_ctrl_amd import BatchControllerEnv
    norm = r.get("norm", True)
    env = BatchControllerEnv(n, r["obs"], r["rew"], norm, norm, r["ct"], r["cm"], reset_ref_mode=r.get("reset"),
                             disturbance_mode=r.get("dist"), tk=r.get("tk", 1.0),
                             sample_time=r.get("sample_time", 0.05), action_max=r.get("action_max", 17 * math.pi / 180),
                             use_limiter=r.get("use_limiter", False), aero_err=r.get("aero_err"), seed=seed,
                             auto_reset=False, variant=variant)
    if r.get("reset") is None:           # explicit per-env state0 and references (as tests/test_gpu_env.py _run)
        rng = np.random.default_rng(seed)
        s0 = np.stack([np.zeros(n), rng.uniform(1000, 11000, n), rng.uniform(100, 265, n), rng.uniform(-20, 20, n),
                       np.zeros(n), rng.uniform(-1e-3, 1e-3, n)], 1)
        env.set_state0(torch.from_numpy(s0))
        env.set_reference(vartheta=torch.from_numpy(rng.uniform(-0.17, 0.17, n)),
                          h=torch.from_numpy(s0[:, 1] + rng.uniform(-500, 500, n)))
        env.reset()
    if r.get("consts"):                  # before the first step: thrust and both PIDs' gains off their defaults
        c = env.consts
        c.P = 300000.0
        for j, f in enumerate((1.25, 0.8, 1.1, 0.9)):
            c.PID_SS[j] *= f
            c.PID_CS[j] *= 2.0 - f
    if r.get("preset"):
        rng = np.random.default_rng(seed + 1)
        for name, lo, hi in (("upid", -0.05, 0.05), ("deltaz", -0.05, 0.05), ("tp", 0.0, 1.0)):
            getattr(env, name).copy_(torch.from_numpy(rng.uniform(lo, hi, n)))
    env.track_episodes(True)
    return env


def _actions(r, row, env):
    a = np.random.default_rng(100 + row).uniform(-1, 1, env.n)
    if "act_scale" in r:
        a = a * np.resize(np.array(r["act_scale"]), env.n)
    if not r.get("norm", True):
        a = a * env.action_max           # the un-normalised action space
    return a.astype(np.float32)


def _steps(env):
    return int(math.ceil(env.tk / env.sample_time - 1e-9))


def _eval_guarded(env, steps, action, signal="state_vartheta", scale=1.0, band=0.05):
    """b747_eval_episodes through the C ABI with y_base and eval_out as views inside larger tensors filled with a
    sentinel: one column of slack on either side, which the launch must leave untouched."""
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.model import SIG
    n, f64 = env.n, torch.float64
    nrow = len(_lib.EVAL_ROWS)
    ybuf = torch.full((3 * n,), SENT, dtype=f64, device=env.device)
    obuf = torch.full(((nrow + 2) * n,), SENT, dtype=f64, device=env.device)
    yb, out = ybuf[n:2 * n], obuf[n:(nrow + 1) * n].view(nrow, n)
    yb.copy_(env.ref[0] * scale)
    y0 = ybuf.clone()
    env.action.copy_(torch.as_tensor(action, dtype=torch.float32).to(env.device).expand(n))
    b = env._batch()
    b.action = env.action.data_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(env._L.b747_eval_episodes(env._bref, env._cref, env._kref, None, int(steps), SIG[signal], float(scale),
                                         p(yb), float(band), float(env.action_space.low), float(env.action_space.high),
                                         p(out), torch.cuda.current_stream(env.device).cuda_stream),
               "b747_eval_episodes")
    torch.cuda.synchronize()
    assert torch.equal(ybuf.view(torch.int64), y0.view(torch.int64)), "y_base or its guard columns were written"
    guard = torch.cat([obuf[:n], obuf[(nrow + 1) * n:]])
    assert bool((guard == SENT).all()), "eval_out's guard columns were written"
    assert not bool((out == SENT).any())
    return {k: out[j].clone() for j, k in enumerate(_lib.EVAL_ROWS)}


def _state(env, extra=None):
    s = {k: getattr(env, k).clone() for k in BUFS}
    s.update(extra or {})
    return s


def _step_loop(env, a, steps, itse=False):
    """steps x step(a) (b747_env_step); every buffer's column as it was after the env's first done (the loop goes
    on stepping a finished env: auto_reset is off), or after the last step for an env that never finished."""
    at = torch.from_numpy(a).to(env.device)
    ended = torch.zeros(env.n, dtype=torch.bool, device=env.device)
    snap = None
    for _ in range(steps):
        env.step(at)
        cur = _state(env, {"itse": env.signal("ITSE")[-1].clone()} if itse else None)
        if snap is None:
            snap = cur
        else:
            upd = ~ended
            for k, v in cur.items():
                m = upd[:, None] if k in ROW_MAJOR else upd
                snap[k] = torch.where(m, v, snap[k])
        ended = ended | env.done
        if bool(ended.all()):
            break
    return snap


# b747o_model (oracle/b747_oracle.h) starts with its parameters and exported signals, all doubles; b747oe_env
# (oracle/b747_oracle_env.c) is the model followed by the reference slots, tp last.  Index in doubles:
_M = dict(Iz=0, P=1, PID_CS=2, PID_SS=6, S=10, c_=16, deltaz=17, g=18, h_zh=19, m0=20, state0=21, ITSE=51, U_com_PID=61)


def _oracle(env, r, a, steps):
    """The same episodes on the CPU oracle: the state, outputs and slots at each env's first done."""
    from b747_rl_ctrl_amd import CtrlMode as M, RewardType as Rw
    n = env.n
    cpu = lambda t: t.cpu().numpy()
    flags = cpu(env.flags)
    orc = O.EnvOracle(n, r["obs"].value, r["rew"].value, None if r["cm"] is None else r["cm"].value, flags,
                      env.norm_obs, env.norm_act, env.use_limiter, env.sample_time, env.tk, env.action_max,
                      env.vartheta_max)
    m64 = orc.mem.view(np.float64).reshape(n, -1)
    d = O.DEFAULT_CONSTS                 # Iz, P, S, c_, g, m0, PID_CS[4], PID_SS[4]: the layout is what _M says
    for name, j in (("Iz", 0), ("P", 1), ("S", 2), ("c_", 3), ("g", 4), ("m0", 5)):
        assert np.all(m64[:, _M[name]] == d[j]), name
        m64[:, _M[name]] = getattr(env.consts, name)
    assert np.all(m64[:, 2:6] == d[6:10]) and np.all(m64[:, 6:10] == d[10:14])
    m64[:, 2:6], m64[:, 6:10] = list(env.consts.PID_CS), list(env.consts.PID_SS)
    orc.reset(cpu(env.state0), cpu(env.ref), cpu(env.ref_kind), cpu(env.aero_err))
    assert np.array_equal(m64[:, 21:27], cpu(env.state0).T)
    if r.get("preset"):                  # (call before the env's first step: the slots as _mk drew them)
        m64[:, _M["U_com_PID"]], m64[:, _M["deltaz"]], m64[:, -1] = cpu(env.upid), cpu(env.deltaz), cpu(env.tp)
    ctrl = (flags & O.F_PID_CS) != 0
    ret = np.zeros(n, np.float32)
    ended = np.zeros(n, bool)
    snap = {}
    for _ in range(steps):
        obs, rew, done = orc.step(a)
        live = ~ended
        ret[live] = (ret[live].astype(np.float64) + rew[live]).astype(np.float32)     # VecMonitor
        X, disc, k, mem = orc.compact_full()
        cur = dict(X=X, disc=disc, k=k, mem=mem, obs=obs.copy(), terminal_obs=obs.copy(),
                   reward=rew.astype(np.float32), done=done.copy(), ep_return=ret.astype(np.float64),
                   ep_final_return=ret.astype(np.float64), itse=m64[:, _M["ITSE"]].copy(),
                   deltaz=m64[:, _M["deltaz"]].copy(), upid=m64[:, _M["U_com_PID"]].copy(), tp=m64[:, -1].copy(),
                   h_zh=m64[:, _M["h_zh"]].copy())
        for key, v in cur.items():
            if key not in snap:
                snap[key] = v
            else:
                m = live[:, None] if key in ROW_MAJOR else live
                snap[key] = np.where(m, v, snap[key])
        ended |= done
        if ended.all():
            break
    # the slots the kernels keep for this configuration (b747_lanes.h env_store); the others have no oracle value
    if r["cm"] != M.ANG_VEL_CONTROL:
        del snap["deltaz"]
    if r["cm"] not in (M.ADD_PROC_CONTROL, M.ADD_DIRECT_CONTROL):
        del snap["upid"]
    if r["rew"] != Rw.TF_REFERENCE:
        del snap["tp"]
    if not ctrl.all():
        del snap["h_zh"]
    return snap


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _bit_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    same = _bits(a) == _bits(b)
    if a.is_floating_point():
        same = same | (a.isnan() & b.isnan())
    return bool(same.all())


def _deviation(x, o):
    """max over the envs of |x - o| as a share of the component's largest magnitude over the batch"""
    x, o = np.asarray(x, np.float64), np.asarray(o, np.float64)
    scale = np.maximum(np.abs(o).max(axis=-1, keepdims=True), 1e-300)
    return (np.abs(x - o) / scale).max(axis=-1)


def _check(ctx, variant, A, ev, B, orc):
    """A: env A's buffers after the launch, ev: its eval rows, B: the step loop's snapshot, orc: the oracle's (FAST)"""
    assert _bit_equal(ev["length"], A["k"].to(torch.float64)), (ctx, "length != k")
    assert _bit_equal(ev["return"], A["ep_return"].to(torch.float64)), (ctx, "return != ep_return")
    dev = {}
    for k in BUFS:
        if variant == "faithful" or k in EXACT:
            assert _bit_equal(A[k], B[k]), (ctx, k)
            continue
        a, b = A[k].cpu().numpy(), B[k].cpu().numpy()
        if k == "ep_stats":              # [count, return sum, length sum]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), (ctx, k)
            a, b, ok = a[1], b[1], "ep_final_return"
        else:
            ok = k
        if ok not in orc:
            assert _bit_equal(A[k], B[k]), (ctx, k, "no oracle value for this slot: equal to the step loop's")
        elif a.dtype == np.float32 and k != "ep_return":
            np.testing.assert_allclose(b, orc[ok], rtol=RTOL, atol=ATOL, err_msg=f"{ctx} step loop {k}")
            np.testing.assert_allclose(a, orc[ok], rtol=RTOL, atol=ATOL, err_msg=f"{ctx} eval {k}")
        else:
            da, db = _deviation(a, orc[ok]), _deviation(b, orc[ok])
            dev[k] = (float(np.max(db)), float(np.max(da)))
            assert np.all(da <= np.maximum(2 * db, FLOOR)), (ctx, k, da, db)
    return dev


@pytest.mark.parametrize("variant", ["faithful", "fast"])
@pytest.mark.parametrize("row", list(range(1, 14)))
def test_state_parity_with_the_step_loop(row, variant):
    from b747_rl_ctrl_amd import CtrlMode
    r = _rows()[row]
    envA, envB = _mk(r, variant), _mk(r, variant)
    a, steps = _actions(r, row, envA), _steps(envA)
    assert envB.kernel() == ("generic" if r.get("consts") else "defc")
    orc = _oracle(envB, r, a, steps) if variant == "fast" else None
    ev = _eval_guarded(envA, steps, a)
    B = _step_loop(envB, a, steps)
    torch.cuda.synchronize()
    nsub = int(envB.cfg.n_sub)
    if row == 10:
        fl = envB.flags.cpu().numpy() & O.F_PID_CS
        assert fl.any() and not fl.all(), "HYBRID resets must mix CS-PID on and off within the batch"
    if row == 11:                        # on the step loop's lengths: the launch has something to freeze
        lens = B["ep_final_len"].cpu().numpy()
        assert bool(B["done"].all()) and len(set(lens.tolist())) >= 3 and (lens == steps).any() and \
            (lens < steps).any(), sorted(set(lens.tolist()))
    else:
        assert bool((B["k"] == steps * nsub).all()) and bool(B["done"].all())
    if r["cm"] == CtrlMode.ANG_VEL_CONTROL:
        assert float(B["deltaz"].abs().max()) > 0
    dev = _check((row, variant), variant, _state(envA), ev, B, orc)
    if variant == "fast":
        print(f"\nrow {row:2d} FAST deviation from the oracle, step loop / eval: "
              + ", ".join(f"{k} {db:.1e} / {da:.1e}" for k, (db, da) in dev.items()))


@pytest.mark.parametrize("variant", ["faithful", "fast"])
def test_itse_row_is_the_last_dll_steps_itse_signal(variant):
    """Row 1 once more with signal recording on in the step loop (which then runs the RECORDING kind)"""
    r = _rows()[1]
    envA, envB = _mk(r, variant), _mk(r, variant)
    envB.record_signals(True)
    assert envB.kernel() == "recording"
    a, steps = _actions(r, 1, envA), _steps(envA)
    ev = _eval_guarded(envA, steps, a)
    B = _step_loop(envB, a, steps, itse=True)
    if variant == "faithful":
        assert _bit_equal(ev["itse"], B["itse"])
        return
    orc = _oracle(envB, r, a, steps)
    da, db = _deviation(ev["itse"].cpu().numpy(), orc["itse"]), _deviation(B["itse"].cpu().numpy(), orc["itse"])
    print(f"\nITSE deviation from the oracle, step loop / eval: {float(db):.1e} / {float(da):.1e}")
    assert da <= max(2 * db, FLOOR), (da, db)


# ------------------------------------------------------------------ 2. the eval rows against the CPU restatement --

N2, TK2, ST2 = 8, 2.0, 0.05
STATE0 = [0, 11000, 250, 0, 0, 0]
REFS2 = [math.radians(d) for d in (5, -5, 10, -10, 2, -2, 7, -7)]
ACT2 = [0.3, -0.3, 0.1, -0.1, 0.2, -0.2, 0.05, 0.0]
CONFIGS = {"manual_direct": (3, 0), "auto": (1, None)}          # CtrlType / CtrlMode values
# signal, scale, y_base, error_band
CASES = {
    "vartheta_deg": ("state_vartheta", 180 / math.pi, [v * 180 / math.pi for v in REFS2], 0.05),
    "wz_band_0.02": ("state_wz", 1.0, [0.0, 0.01, -0.01, 0.02, -0.02, 0.005, -0.005, 0.03], 0.02),
    "alpha_negative": ("alpha", 1.0, [-0.02 - 0.005 * j for j in range(N2)], 0.05),
}

_cpu_cache = {}


def _cpu_episodes(config):
    """One CPU episode per env (computed once per configuration): time, the three scored signals after every DLL
    step, the per-step rewards and the model's ITSE at the end"""
    if config not in _cpu_cache:
        ct, cm = CONFIGS[config]
        eps = []
        for vref, a in zip(REFS2, ACT2):
            c = R.RefController(ct, cm, None, None, tk=TK2, sample_time=ST2)
            e = R.RefControllerEnv(0, 0, True, True, c)
            e.reset({"state0": np.array(STATE0, float), "kind": "const", "ref": vref, "aero_err": None})
            alpha = ctypes.c_double.in_dll(c.model._dll, "alpha")
            ep = {"t": [], "state_vartheta": [], "state_wz": [], "alpha": [], "rewards": []}

            def rec(m, ep=ep, alpha=alpha):
                ep["t"].append(m.time)
                ep["state_vartheta"].append(float(m.state[4]))          # (the state getter's nan_to_num)
                ep["state_wz"].append(float(m.state[5]))
                ep["alpha"].append(float(np.nan_to_num(alpha.value)))
            done = False
            while not done:
                _, rew, done = e.step(np.float32(a), rec)
                ep["rewards"].append(rew)
            ep["itse"] = c.model.ITSE
            eps.append(ep)
        _cpu_cache[config] = eps
    return _cpu_cache[config]


@pytest.mark.parametrize("variant", ["faithful", "fast"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_eval_rows_against_the_cpu_restatement(config, case, variant):
    """Tolerances of the four step-info rows: tests/test_gpu_evaluate.py's (overshoot 1e-3 relative, rise / settling
    time within one DLL sample, static error 1e-5, NaN exactly where calc_stepinfo gives None); itse 1e-6 relative
    (the project's quality tolerance); length exact.
    The return row: VecMonitor's accumulation ret <- float32(float64(ret) + r) of the CPU episode's rewards.  The
    project holds every float32 reward to |r_gpu - r_cpu| <= 2e-6 |r| + 1e-7 (tests/test_gpu_env.py); the float64
    sums of `steps` such rewards then differ by at most steps * (2e-6 max|r| + 1e-7), and each of the two float32
    roundings per step moves a sum by at most half an ulp of the return, which either accumulates on both sides alike
    or is absorbed into the next rounding: one float32 ulp of the return on top."""
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, RewardType
    ct, cm = CONFIGS[config]
    signal, scale, y_base, band = CASES[case]
    env = BatchControllerEnv(N2, ObservationType.PID_LIKE, RewardType.CLASSIC, True, True, CtrlType(ct),
                             None if cm is None else CtrlMode(cm), tk=TK2, sample_time=ST2, auto_reset=False,
                             state0=STATE0, variant=variant)
    env.set_reference(vartheta=torch.tensor(REFS2, dtype=torch.float64))
    env.reset()
    ev = env.eval_episodes(_steps(env), None, signal, scale=scale, y_base=y_base, error_band=band,
                           action=torch.tensor(ACT2))
    torch.cuda.synchronize()
    assert bool(env.done.all())
    ev = {k: v.cpu().numpy() for k, v in ev.items()}
    for j, ep in enumerate(_cpu_episodes(config)):
        ctx = (config, case, variant, j)
        info = calc_stepinfo([scale * y for y in ep[signal]], y_base[j], error_band=band, ts=ep["t"])
        assert int(ev["length"][j]) == len(ep["t"]) == 200, ctx
        if info["overshoot"] is None:
            assert y_base[j] == 0 and math.isnan(ev["overshoot"][j]), ctx
        else:
            assert ev["overshoot"][j] == pytest.approx(info["overshoot"], rel=1e-3), ctx
        for k in ("rise_time", "settling_time"):
            if info[k] is None:
                assert math.isnan(ev[k][j]), (ctx, k)
            else:
                assert abs(ev[k][j] - info[k]) <= 0.0100001, (ctx, k, ev[k][j], info[k])
        assert ev["static_error"][j] == pytest.approx(info["static_error"], abs=1e-5), ctx
        assert ev["itse"][j] == pytest.approx(ep["itse"], rel=1e-6), ctx
        ret = np.float32(0.0)
        for rew in ep["rewards"]:
            ret = np.float32(np.float64(ret) + rew)
        bound = len(ep["rewards"]) * (RTOL * max(abs(x) for x in ep["rewards"]) + ATOL) + float(np.spacing(ret))
        assert abs(ev["return"][j] - float(ret)) <= bound, (ctx, ev["return"][j], float(ret), bound)


# ------------------------------------------------------------------ 3. edges of the launch itself --

@pytest.mark.parametrize("row", [1, 3, 5, 6, 8])
def test_truncated_launch_then_a_second_call(row):
    """Rows 3, 5, 6 and 8 as well as 1: the second call starts from the slots (upid, deltaz, tp, h_zh) and the
    ep_return the first one stored"""
    r = _rows()[row]
    env1, env2, envB = (_mk(r, "faithful") for _ in range(3))
    a, steps, nsub = _actions(r, row, env1), _steps(env1), int(env1.cfg.n_sub)
    n1 = 8
    first = _eval_guarded(env1, n1, a)
    assert not bool(env1.done.any()) and bool((first["length"] == n1 * nsub).all())
    assert bool((env1.k == n1 * nsub).all()) and bool((env1.ep_stats == 0).all())
    second = _eval_guarded(env1, steps - n1, a)
    whole = _eval_guarded(env2, steps, a)
    B = _step_loop(envB, a, steps)
    assert bool(env1.done.all()) and bool((second["length"] == (steps - n1) * nsub).all())
    for k in ("itse", "return"):
        assert _bit_equal(second[k], whole[k]), k
    S1, S2 = _state(env1), _state(env2)
    for k in BUFS:
        assert _bit_equal(S1[k], S2[k]), ("two launches / one", k)
        assert _bit_equal(S1[k], B[k]), ("two launches / step loop", k)


def _saturated_policy(obs_dim, sign):
    """Every weight zero, the action net's bias far outside the action range: mean = sign * 1000 whatever the obs"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    net = ActorCritic(obs_dim)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        net.action_net.bias.fill_(sign * 1000.0)
    return net


@pytest.mark.parametrize("lo,hi", [(-1.0, 1.0), (-0.5, 0.25)])
@pytest.mark.parametrize("obs", ["PID_LIKE", "SPEED_MODE"])
def test_policy_path_clips_and_feeds_the_env_as_the_held_action_path(obs, lo, hi):
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, RewardType
    from b747_rl_ctrl_amd.evaluate import packed_policy

    def mk():
        env = BatchControllerEnv(N2, ObservationType[obs], RewardType.CLASSIC, True, True, CtrlType.MANUAL,
                                 CtrlMode.DIRECT_CONTROL, tk=1.0, sample_time=ST2, auto_reset=False, state0=STATE0,
                                 variant="faithful")
        env.set_reference(vartheta=torch.tensor(REFS2, dtype=torch.float64))
        env.reset()
        env.track_episodes(True)
        return env
    for sign, bound in ((1.0, hi), (-1.0, lo)):
        assert float(np.float32(bound)) == bound
        envP, envH = mk(), mk()
        kw = dict(signal="state_vartheta", scale=180 / math.pi, act_lo=lo, act_hi=hi)
        evP = envP.eval_episodes(_steps(envP), packed_policy(_saturated_policy(envP.obs_dim, sign), envP.obs_dim,
                                                             envP.device), **kw)
        evH = envH.eval_episodes(_steps(envH), None, action=bound, **kw)
        torch.cuda.synchronize()
        assert bool(envP.done.all())
        for k in ("return", "length", "itse"):
            assert _bit_equal(evP[k], evH[k]), (sign, k)
        SP, SH = _state(envP), _state(envH)
        for k in BUFS:
            assert _bit_equal(SP[k], SH[k]), (sign, k)
