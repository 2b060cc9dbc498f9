"""b747_ppo_update_workspace / b747_ppo_grad / b747_ppo_adam (include/b747.h, ABI 12): bound, and their argument
validation -- nothing here launches or touches a GPU (as tests/test_abi.py: the entry points refuse bad arguments
before they reach the device; the pointers below are never dereferenced)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue
PTR = ctypes.c_void_p(0x1000)

GRAD_ARGS = ("theta", "obs_dim", "obs", "act", "old_logp", "adv", "ret", "idx", "batch", "clip_range", "ent_coef",
             "vf_coef", "workspace", "grad", "stats", "stream")
ADAM_ARGS = ("theta", "m", "v", "t", "grad", "n_params", "grad_scale", "max_grad_norm", "lr", "beta1", "beta2", "eps",
             "stream")


def _lib():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


def _grad_args(**over):
    a = dict(theta=PTR, obs_dim=3, obs=PTR, act=PTR, old_logp=PTR, adv=PTR, ret=PTR, idx=PTR, batch=64, clip_range=0.2,
             ent_coef=0.0, vf_coef=0.5, workspace=PTR, grad=PTR, stats=PTR, stream=None)
    a.update(over)
    return [a[k] for k in GRAD_ARGS]


def _adam_args(**over):
    a = dict(theta=PTR, m=PTR, v=PTR, t=PTR, grad=PTR, n_params=8963, grad_scale=1.0, max_grad_norm=0.5, lr=3e-4,
             beta1=0.9, beta2=0.999, eps=1e-5, stream=None)
    a.update(over)
    return [a[k] for k in ADAM_ARGS]


def test_the_update_entry_points_are_bound():
    lib, L = _lib()
    assert lib.ABI_VERSION >= 12
    for name in ("b747_ppo_update_workspace", "b747_ppo_grad", "b747_ppo_adam"):
        assert name in lib.SIGNATURES and hasattr(L, name)
    assert len(lib.SIGNATURES["b747_ppo_grad"][0]) == len(GRAD_ARGS)
    assert len(lib.SIGNATURES["b747_ppo_adam"][0]) == len(ADAM_ARGS)


def test_workspace_is_positive_and_grows_with_obs_dim():
    _, L = _lib()
    sizes = [int(L.b747_ppo_update_workspace(od)) for od in (3, 5, 7, 8, 10)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)), sizes
    # one partial gradient vector per workgroup: the growth is a whole number of 128-float rows (2 nets x 64 units)
    assert (sizes[1] - sizes[0]) % (2 * 128 * 4) == 0
    for od in (0, 1, 4, 6, 9, 11, -3):
        assert L.b747_ppo_update_workspace(od) == INVALID and b"obs_dim" in L.b747_last_error()


@pytest.mark.parametrize("field", ["theta", "obs", "act", "old_logp", "adv", "ret", "idx", "workspace", "grad", "stats"])
def test_grad_rejects_null_pointers_by_name(field):
    _, L = _lib()
    assert L.b747_ppo_grad(*_grad_args(**{field: None})) == INVALID
    assert field.encode() in L.b747_last_error() and b"NULL" in L.b747_last_error(), L.b747_last_error()


@pytest.mark.parametrize("od", [0, 4, 6, 9, 11])
def test_grad_rejects_unsupported_obs_dim(od):
    _, L = _lib()
    assert L.b747_ppo_grad(*_grad_args(obs_dim=od)) == INVALID and b"obs_dim" in L.b747_last_error()


@pytest.mark.parametrize("batch", [1, 0, -5])
def test_grad_rejects_a_batch_below_two(batch):
    _, L = _lib()
    assert L.b747_ppo_grad(*_grad_args(batch=batch)) == INVALID and b"batch" in L.b747_last_error()


@pytest.mark.parametrize("field", ["theta", "m", "v", "t", "grad"])
def test_adam_rejects_null_pointers_by_name(field):
    _, L = _lib()
    assert L.b747_ppo_adam(*_adam_args(**{field: None})) == INVALID
    assert (field + " is NULL").encode() in L.b747_last_error(), L.b747_last_error()


def test_adam_rejects_an_empty_vector():
    _, L = _lib()
    assert L.b747_ppo_adam(*_adam_args(n_params=0)) == INVALID and b"n_params" in L.b747_last_error()
