"""b747_ppo_gae / b747_ppo_epoch / b747_get_specialization (include/b747.h, ABI 13): bound, and their argument
validation -- nothing here launches or touches a GPU (as tests/test_ppo_update_abi.py: the entry points refuse bad
arguments before they reach the device; the pointers below are never dereferenced)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue
PTR = ctypes.c_void_p(0x1000)

GAE_ARGS = ("rew", "val", "done", "last_value", "T", "N", "gamma", "gae_lambda", "adv", "ret", "stream")
EPOCH_ARGS = ("theta", "obs_dim", "obs", "act", "old_logp", "adv", "ret", "perm", "n_rows", "batch_size", "clip_range",
              "ent_coef", "vf_coef", "workspace", "grad", "m", "v", "t", "max_grad_norm", "lr", "beta1", "beta2", "eps",
              "stats", "stream")


def _lib():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


def _gae_args(**over):
    a = dict(rew=PTR, val=PTR, done=PTR, last_value=PTR, T=16, N=64, gamma=0.99, gae_lambda=0.95, adv=PTR, ret=PTR,
             stream=None)
    a.update(over)
    return [a[k] for k in GAE_ARGS]


def _epoch_args(**over):
    a = dict(theta=PTR, obs_dim=3, obs=PTR, act=PTR, old_logp=PTR, adv=PTR, ret=PTR, perm=PTR, n_rows=1024,
             batch_size=300, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, workspace=PTR, grad=PTR, m=PTR, v=PTR, t=PTR,
             max_grad_norm=0.5, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, stats=PTR, stream=None)
    a.update(over)
    return [a[k] for k in EPOCH_ARGS]


def test_the_entry_points_are_bound():
    lib, L = _lib()
    assert lib.ABI_VERSION >= 13 and int(L.b747_abi_version()) == lib.ABI_VERSION
    for name in ("b747_ppo_gae", "b747_ppo_epoch", "b747_get_specialization"):
        assert name in lib.SIGNATURES and hasattr(L, name)
    assert len(lib.SIGNATURES["b747_ppo_gae"][0]) == len(GAE_ARGS)
    assert len(lib.SIGNATURES["b747_ppo_epoch"][0]) == len(EPOCH_ARGS)
    assert lib.SIGNATURES["b747_get_specialization"][0] == []


@pytest.mark.parametrize("field", ["rew", "val", "done", "last_value", "adv", "ret"])
def test_gae_rejects_null_pointers_by_name(field):
    _, L = _lib()
    assert L.b747_ppo_gae(*_gae_args(**{field: None})) == INVALID
    assert (field + " is NULL").encode() in L.b747_last_error(), L.b747_last_error()


@pytest.mark.parametrize("field", ["T", "N"])
def test_gae_rejects_negative_sizes(field):
    _, L = _lib()
    assert L.b747_ppo_gae(*_gae_args(**{field: -1})) == INVALID
    assert (field + " < 0").encode() in L.b747_last_error(), L.b747_last_error()


def test_gae_of_nothing_returns_zero_and_launches_nothing():
    _, L = _lib()
    assert L.b747_ppo_gae(*_gae_args(T=0)) == 0        # (no GPU here: a launch would have failed)
    assert L.b747_ppo_gae(*_gae_args(N=0)) == 0


@pytest.mark.parametrize("field", ["theta", "obs", "act", "old_logp", "adv", "ret", "perm", "workspace", "grad", "m", "v",
                                   "t", "stats"])
def test_epoch_rejects_null_pointers_by_name(field):
    _, L = _lib()
    assert L.b747_ppo_epoch(*_epoch_args(**{field: None})) == INVALID
    assert (field + " is NULL").encode() in L.b747_last_error(), L.b747_last_error()


@pytest.mark.parametrize("od", [0, 4, 6, 9, 11])
def test_epoch_rejects_unsupported_obs_dim(od):
    _, L = _lib()
    assert L.b747_ppo_epoch(*_epoch_args(obs_dim=od)) == INVALID and b"obs_dim" in L.b747_last_error()


@pytest.mark.parametrize("n_rows", [1, 0, -4])
def test_epoch_rejects_fewer_than_two_rows(n_rows):
    _, L = _lib()
    assert L.b747_ppo_epoch(*_epoch_args(n_rows=n_rows)) == INVALID and b"n_rows < 2" in L.b747_last_error()


@pytest.mark.parametrize("batch_size", [1, 0, -4])
def test_epoch_rejects_a_batch_size_below_two(batch_size):
    _, L = _lib()
    assert L.b747_ppo_epoch(*_epoch_args(batch_size=batch_size)) == INVALID
    assert b"batch_size < 2" in L.b747_last_error(), L.b747_last_error()


@pytest.mark.parametrize("n_rows,batch_size", [(1024, 1023), (1025, 64), (3, 2)])
def test_epoch_rejects_a_last_minibatch_of_one_row(n_rows, batch_size):
    _, L = _lib()
    assert L.b747_ppo_epoch(*_epoch_args(n_rows=n_rows, batch_size=batch_size)) == INVALID
    assert b"n_rows % batch_size == 1" in L.b747_last_error(), L.b747_last_error()


def test_get_specialization_reads_the_switch_and_changes_nothing():
    _, L = _lib()
    prev = int(L.b747_get_specialization())
    assert prev in (0, 1, 2)
    try:
        for on in (0, 1, 2, 1, 0):
            L.b747_set_specialization(on)
            assert L.b747_get_specialization() == on
            assert L.b747_get_specialization() == on                # a read leaves it
        assert L.b747_set_specialization(2) == 0 and L.b747_get_specialization() == 2
    finally:
        L.b747_set_specialization(prev)
    assert L.b747_get_specialization() == prev
