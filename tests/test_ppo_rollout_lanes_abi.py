"""b747_ppo_rollout_lanes (include/b747.h, ABI 14): bound, its argument validation, and its coverage -- each of the 18
configurations the reference's main.py trains (2 observation types x 3 control modes x 3 reset modes, no disturbance,
sample_time 0.05) is accepted by it and refused by b747_ppo_rollout.  Nothing here launches or touches a GPU (as
tests/test_ppo_epoch_abi.py: the entry points refuse bad arguments before they reach the device, T = 0 validates and
launches nothing; the pointers below are never dereferenced)."""
import ctypes
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue
PTR = 0x1000

ARGS = ("b", "cfg", "c", "params", "seed", "step_base", "T", "obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf",
        "done_buf", "act_lo", "act_hi", "stream")
OBS_PID_LIKE, OBS_SPEED_MODE, OBS_MODEL_STATE = 0, 1, 4
REW_CLASSIC = 0
MODE_DIRECT, MODE_ADD_PROC, MODE_ADD_DIRECT = 0, 1, 3
RESET_CONST, RESET_OSCILLATING, RESET_HYBRID = 0, 1, 2
# main.py:7-12 ctrl_mode_max
ACTION_MAX = {MODE_DIRECT: 17 * math.pi / 180, MODE_ADD_PROC: 1.0, MODE_ADD_DIRECT: 10 * math.pi / 180}
MAIN_PY = [(o, m, r) for o in (OBS_PID_LIKE, OBS_SPEED_MODE) for m in (MODE_DIRECT, MODE_ADD_DIRECT, MODE_ADD_PROC)
           for r in (RESET_CONST, RESET_OSCILLATING, RESET_HYBRID)]


def _lib():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


def _env(obs_type=OBS_PID_LIKE, ctrl_mode=MODE_DIRECT, reset=RESET_CONST, disturbance=-1, n=70, x_f64=1, sig=None,
         variant=0):
    """A batch descriptor of dummy pointers with main.py's settings (MANUAL, CLASSIC, normalised, sample_time 0.05)"""
    lib, L = _lib()
    cfg = lib.EnvConfig()
    assert L.b747_env_config_default(ctypes.byref(cfg), obs_type, REW_CLASSIC) == 0
    cfg.ctrl_mode, cfg.reset_ref_mode, cfg.disturbance_mode = ctrl_mode, reset, disturbance
    cfg.n_sub, cfg.sample_time, cfg.tk, cfg.action_max = 5, 0.05, 20.0, ACTION_MAX[ctrl_mode]
    b = lib.EnvBatch()
    b.n, b.env_offset, b.x_f64, b.obs_dim, b.variant = n, 0, x_f64, int(L.b747_env_obs_dim(obs_type)), variant
    for f in lib._ENV_PTRS:
        setattr(b, f, PTR)
    b.sig, b.rec_params = sig, None
    return b, cfg, lib.default_consts()


def _args(env=None, **over):
    b, cfg, c = env or _env()
    a = dict(b=ctypes.byref(b), cfg=ctypes.byref(cfg), c=ctypes.byref(c), params=PTR, seed=1, step_base=PTR, T=16,
             obs_buf=PTR, act_buf=PTR, logp_buf=PTR, val_buf=PTR, rew_buf=PTR, done_buf=PTR, act_lo=-1.0, act_hi=1.0,
             stream=None)
    a.update(over)
    return [a[k] for k in ARGS], (b, cfg, c)   # (the structures stay referenced while the call runs)


def _refused(L, args, word):
    a, keep = args
    assert L.b747_ppo_rollout_lanes(*a) == INVALID
    assert word.encode() in L.b747_last_error(), L.b747_last_error()


def test_the_entry_point_is_bound():
    lib, L = _lib()
    assert lib.ABI_VERSION >= 14 and int(L.b747_abi_version()) == lib.ABI_VERSION
    assert "b747_ppo_rollout_lanes" in lib.SIGNATURES and hasattr(L, "b747_ppo_rollout_lanes")
    assert lib.SIGNATURES["b747_ppo_rollout_lanes"] == lib.SIGNATURES["b747_ppo_rollout"]   # the same arguments
    assert len(lib.SIGNATURES["b747_ppo_rollout_lanes"][0]) == len(ARGS)


@pytest.mark.parametrize("field", ["params", "obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf"])
def test_rejects_null_buffers_by_name(field):
    _, L = _lib()
    _refused(L, _args(**{field: None}), field + " is NULL")


def test_rejects_null_consts():
    _, L = _lib()
    _refused(L, _args(c=None), "consts is NULL")


def test_rejects_a_negative_step_count():
    _, L = _lib()
    _refused(L, _args(T=-1), "T < 0")


def test_rejects_an_empty_action_range():
    _, L = _lib()
    _refused(L, _args(act_lo=0.5, act_hi=-0.5), "act_lo > act_hi")
    _refused(L, _args(act_lo=float("nan")), "act_lo > act_hi")


@pytest.mark.parametrize("obs_type,od", [(2, 8), (3, 10), (OBS_MODEL_STATE, 7)])
def test_rejects_other_observation_types(obs_type, od):
    _, L = _lib()
    env = _env(obs_type=obs_type)
    assert env[0].obs_dim == od
    for T in (0, 16):    # (refused before anything would launch)
        _refused(L, _args(env, T=T), "obs_dim")


def test_rejects_fp32_state():
    _, L = _lib()
    _refused(L, _args(_env(x_f64=0), T=0), "x_f64")


def test_rejects_a_recording_batch():
    _, L = _lib()
    _refused(L, _args(_env(sig=PTR), T=0), "sig")


@pytest.mark.parametrize("obs_type,ctrl_mode,reset", MAIN_PY)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_covers_every_main_py_configuration_that_the_split_kernel_refuses(obs_type, ctrl_mode, reset, variant):
    _, L = _lib()
    for n in (1, 4, 70, 65536):
        a, keep = _args(_env(obs_type, ctrl_mode, reset, n=n, variant=variant), T=0)
        assert L.b747_ppo_rollout_lanes(*a) == 0, L.b747_last_error()
        assert L.b747_ppo_rollout(*a) == INVALID and b"training configuration only" in L.b747_last_error()


def test_covers_the_bench_configuration_and_an_empty_batch():
    _, L = _lib()
    a, keep = _args(_env(disturbance=0, n=64), T=0)
    assert L.b747_ppo_rollout_lanes(*a) == 0 and L.b747_ppo_rollout(*a) == 0
    a, keep = _args(_env(n=0), T=16)
    assert L.b747_ppo_rollout_lanes(*a) == 0
