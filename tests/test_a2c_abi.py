"""b747_a2c_grad / b747_ppo_rmsprop / b747_a2c_update (include/b747.h, additive under ABI 15): declared, bound, and their
argument validation -- nothing here launches or touches a GPU (as tests/test_ppo_update_abi.py: the entry points refuse
bad arguments before they reach the device; the pointers below are never dereferenced).  A2CConfig's defaults with them."""
import ctypes
import math
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue
PTR = ctypes.c_void_p(0x1000)

GRAD_ARGS = ("theta", "obs_dim", "obs", "act", "adv", "ret", "idx", "batch", "normalize_advantage", "ent_coef", "vf_coef",
             "workspace", "grad", "stats", "stream")
RMS_ARGS = ("theta", "sq", "t", "grad", "n_params", "grad_scale", "max_grad_norm", "lr", "alpha", "eps", "tf_like",
            "stream")
UPDATE_ARGS = GRAD_ARGS[:-1] + ("optimizer", "state0", "state1", "t", "max_grad_norm", "lr", "alpha", "eps", "stream")
ARGS = {"b747_a2c_grad": GRAD_ARGS, "b747_ppo_rmsprop": RMS_ARGS, "b747_a2c_update": UPDATE_ARGS}


def _lib():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


def _args(name, **over):
    a = dict(theta=PTR, obs_dim=3, obs=PTR, act=PTR, adv=PTR, ret=PTR, idx=PTR, batch=64, normalize_advantage=0,
             ent_coef=0.0, vf_coef=0.5, workspace=PTR, grad=PTR, stats=PTR, stream=None, sq=PTR, t=PTR, n_params=8963,
             grad_scale=1.0, max_grad_norm=0.5, lr=7e-4, alpha=0.99, eps=1e-5, tf_like=0, optimizer=1, state0=PTR,
             state1=PTR)
    assert set(over) <= set(ARGS[name]), over
    a.update(over)
    return [a[k] for k in ARGS[name]]


def _refused(name, needle, **over):
    _, L = _lib()
    assert getattr(L, name)(*_args(name, **over)) == INVALID, (name, over)
    msg = L.b747_last_error()
    assert needle.encode() in msg and name.encode() in msg, msg


def _header():
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(ARGS))
def test_the_entry_points_are_declared_and_bound_with_matching_arity(name):
    lib, L = _lib()
    assert name in lib.SIGNATURES and hasattr(L, name)
    m = re.search(r"int32_t " + name + r"\(([^;]*)\);", _header())
    assert m, name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    names = tuple(p.split()[-1].lstrip("*") for p in params)
    assert names == ARGS[name]
    assert len(lib.SIGNATURES[name][0]) == len(ARGS[name])


def test_the_optimizer_values_agree_with_the_header():
    lib, _ = _lib()
    h = _header()
    for name in ("ADAM", "RMSPROP", "RMSPROP_TF"):
        m = re.search(r"#define B747_OPT_" + name + r" (\d+)\s", h)
        assert m and int(m.group(1)) == getattr(lib, "OPT_" + name), name
    from b747_rl_ctrl_amd.ppo import A2C_OPTIMIZERS
    assert [A2C_OPTIMIZERS.index(k) for k in ("adam", "rmsprop", "rmsprop_tf")] == \
        [lib.OPT_ADAM, lib.OPT_RMSPROP, lib.OPT_RMSPROP_TF]


@pytest.mark.parametrize("name", ["b747_a2c_grad", "b747_a2c_update"])
@pytest.mark.parametrize("field", ["theta", "obs", "act", "adv", "ret", "workspace", "grad", "stats"])
def test_the_row_calls_reject_null_pointers_by_name(name, field):
    _refused(name, field + " is NULL", **{field: None})


@pytest.mark.parametrize("field", ["theta", "sq", "t", "grad"])
def test_rmsprop_rejects_null_pointers_by_name(field):
    _refused("b747_ppo_rmsprop", field + " is NULL", **{field: None})


def test_update_rejects_null_state_by_name():
    _refused("b747_a2c_update", "state0 is NULL", state0=None)
    _refused("b747_a2c_update", "t is NULL", t=None)
    _refused("b747_a2c_update", "state1 is NULL", optimizer=0, state1=None)      # Adam's v


@pytest.mark.parametrize("name", ["b747_a2c_grad", "b747_a2c_update"])
def test_the_row_calls_reject_obs_dim_and_batch(name):
    for od in (0, 4, 6, 9, 11):
        _refused(name, "obs_dim", obs_dim=od)
    for batch in (0, -5):
        _refused(name, "batch", batch=batch)
    _refused(name, "batch", batch=1, normalize_advantage=1)


@pytest.mark.parametrize("field", ["lr", "eps", "max_grad_norm"])
@pytest.mark.parametrize("value", [0.0, -1.0, math.inf, math.nan])
def test_the_optimiser_calls_reject_scalars_that_are_not_finite_and_positive(field, value):
    _refused("b747_ppo_rmsprop", field, **{field: value})
    for opt in (0, 1, 2):
        _refused("b747_a2c_update", field, optimizer=opt, **{field: value})


@pytest.mark.parametrize("alpha", [-0.1, 1.0, 1.5, math.nan])
def test_alpha_outside_the_half_open_unit_interval(alpha):
    _refused("b747_ppo_rmsprop", "alpha", alpha=alpha)
    _refused("b747_a2c_update", "alpha", optimizer=1, alpha=alpha)
    _refused("b747_a2c_update", "alpha", optimizer=2, alpha=alpha)


def test_rmsprop_rejects_an_empty_vector_and_update_an_unknown_optimizer():
    _refused("b747_ppo_rmsprop", "n_params", n_params=0)
    for opt in (-1, 3, 17):
        _refused("b747_a2c_update", "optimizer", optimizer=opt)


def test_a_null_idx_passes_validation():
    """idx = NULL is the identity order: with it and a later argument wrong, the later argument is what is named (the
    call never reaches the device)"""
    _, L = _lib()
    assert L.b747_a2c_grad(*_args("b747_a2c_grad", idx=None, stats=None)) == INVALID
    assert b"stats is NULL" in L.b747_last_error() and b"idx" not in L.b747_last_error()
    assert L.b747_a2c_update(*_args("b747_a2c_update", idx=None, optimizer=9)) == INVALID
    assert b"optimizer" in L.b747_last_error() and b"idx" not in L.b747_last_error()
    # batch = 1 is a batch without normalize_advantage
    assert L.b747_a2c_grad(*_args("b747_a2c_grad", idx=None, batch=1, stats=None)) == INVALID
    assert b"stats is NULL" in L.b747_last_error()


def test_the_source_is_a_translation_unit_of_its_own():
    from b747_rl_ctrl_amd import build
    assert any(s.endswith("b747_a2c_update.hip") for s in build.SOURCES)


def test_a2c_config_defaults_and_the_reference_entry():
    from b747_rl_ctrl_amd.ppo import A2CConfig
    c = A2CConfig()
    assert (c.n_steps, c.gamma, c.gae_lambda, c.ent_coef, c.vf_coef, c.max_grad_norm, c.learning_rate) == \
        (5, 0.99, 1.0, 0.0, 0.5, 0.5, 7e-4)                  # SB3 1.4 A2C.__init__
    assert (c.normalize_advantage, c.optimizer, c.rms_alpha, c.rms_eps) == (False, "rmsprop", 0.99, 1e-5)
    r = A2CConfig.reference()                                # neural/setups.py hyperparams[A2C]
    assert (r.optimizer, r.rms_eps, r.rms_alpha) == ("rmsprop_tf", 1e-9, 0.99)
    assert {k: v for k, v in vars(r).items() if k not in ("optimizer", "rms_eps")} == \
        {k: v for k, v in vars(c).items() if k not in ("optimizer", "rms_eps")}
