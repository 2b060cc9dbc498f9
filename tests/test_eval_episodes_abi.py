"""b747_eval_episodes (include/b747.h, ABI 11): bound, and its argument validation -- no launch, no GPU (as
tests/test_abi.py: the entry points refuse bad arguments before they touch the device)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue


def _setup(obs_type=0):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    b, cfg = _lib.EnvBatch(), _lib.EnvConfig()
    assert L.b747_env_config_default(ctypes.byref(cfg), obs_type, 0) == 0
    cfg.auto_reset = 0
    b.n, b.x_f64, b.obs_dim = 4, 1, L.b747_env_obs_dim(obs_type)
    for f in _lib._ENV_PTRS:          # never dereferenced: nothing below launches
        setattr(b, f, 0x1000)
    return _lib, L, b, cfg


def _call(L, _lib, b, cfg, params, n_env_steps=0):
    p = ctypes.c_void_p
    return L.b747_eval_episodes(ctypes.byref(b), ctypes.byref(cfg), ctypes.byref(_lib.default_consts()), params,
                                n_env_steps, 9, 180 / 3.141592653589793, p(0x1000), 0.05, -1.0, 1.0, p(0x1000), None)


def test_eval_episodes_is_bound_and_validates_without_launching():
    _lib, L, b, cfg = _setup()
    assert "b747_eval_episodes" in _lib.SIGNATURES and _lib.ABI_VERSION >= 11 and len(_lib.EVAL_ROWS) == 7
    assert _call(L, _lib, b, cfg, None) == 0                        # T = 0: valid, launches nothing
    assert _call(L, _lib, b, cfg, ctypes.c_void_p(0x1000)) == 0     # with a policy, PID_LIKE (obs_dim 3)
    _lib5, L5, b5, cfg5 = _setup(obs_type=1)
    assert _call(L5, _lib5, b5, cfg5, ctypes.c_void_p(0x1000)) == 0  # SPEED_MODE (obs_dim 5)


@pytest.mark.parametrize("case,word", [("auto_reset", b"auto_reset"), ("fp32_state", b"x_f64"), ("obs_dim_7", b"obs_dim")])
def test_eval_episodes_rejects_what_the_kernel_does_not_cover(case, word):
    _lib, L, b, cfg = _setup(obs_type=4 if case == "obs_dim_7" else 0)
    params = None
    if case == "auto_reset":
        cfg.auto_reset = 1
    elif case == "fp32_state":
        b.x_f64 = 0
    else:
        assert b.obs_dim == 7
        params = ctypes.c_void_p(0x1000)
    for steps in (0, 10):
        assert _call(L, _lib, b, cfg, params, steps) == INVALID
        assert word in L.b747_last_error(), L.b747_last_error()
    if case == "obs_dim_7":                                         # the same observation type without a policy is fine
        assert _call(L, _lib, b, cfg, None) == 0


def test_eval_episodes_rejects_bad_rows_and_null_buffers():
    _lib, L, b, cfg = _setup()
    p = ctypes.c_void_p
    k = ctypes.byref(_lib.default_consts())
    assert L.b747_eval_episodes(ctypes.byref(b), ctypes.byref(cfg), k, None, 0, 31, 1.0, p(0x1000), 0.05, -1.0, 1.0,
                                p(0x1000), None) == INVALID and b"sig_row" in L.b747_last_error()
    assert L.b747_eval_episodes(ctypes.byref(b), ctypes.byref(cfg), k, None, 0, 9, 1.0, None, 0.05, -1.0, 1.0,
                                p(0x1000), None) == INVALID and b"NULL" in L.b747_last_error()
    assert L.b747_eval_episodes(ctypes.byref(b), ctypes.byref(cfg), k, None, -1, 9, 1.0, p(0x1000), 0.05, -1.0, 1.0,
                                p(0x1000), None) == INVALID
    b.action = None
    assert _call(L, _lib, b, cfg, None) == INVALID and b"action" in L.b747_last_error()
