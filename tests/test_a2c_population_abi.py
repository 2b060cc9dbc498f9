"""b747_a2c_update_population (include/b747.h, additive under ABI 15): declared, bound, the optimiser
column of the hyper-parameter table, and the argument validation -- nothing here launches or touches a GPU (as
tests/test_a2c_abi.py: the entry point refuses bad arguments before they reach the device; the pointers below are never
dereferenced).  ppo.a2c_hyper_table with them."""
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
NAME = "b747_a2c_update_population"
ARGS = ("theta", "n_policies", "policy_stride", "obs_dim", "obs", "act", "adv", "ret", "rows", "rows_stride", "batch",
        "normalize_advantage", "hyper_dev", "workspace", "workspace_bytes", "state0", "state1", "t", "rms_alpha",
        "rms_eps", "adam_beta1", "adam_beta2", "adam_eps", "stats", "stream")
POINTERS = ("theta", "obs", "act", "adv", "ret", "rows", "hyper_dev", "workspace", "state0", "state1", "t", "stats")


def _lib():
    from b747_rl_ctrl_amd import _lib
    return _lib, _lib.lib()


def _header():
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        return f.read()


def _slice_bytes(od, batch):
    """upd_pop_ws_bytes (csrc/b747_ppo_update.h), as tests/test_ppo_population_hyper_abi.py writes it"""
    n_wg = min(256, -(-(-(-batch // 32)) // 2))
    n_params = 128 * od + 8579
    return -(-(1024 + 72 * n_wg + 4 * n_params * (n_wg + 1)) // 16) * 16


def _args(L, **over):
    a = dict(theta=PTR, n_policies=3, policy_stride=int(L.b747_policy_num_params(3)), obs_dim=3, obs=PTR, act=PTR,
             adv=PTR, ret=PTR, rows=PTR, rows_stride=320, batch=320, normalize_advantage=0, hyper_dev=PTR,
             workspace=PTR, workspace_bytes=3 * _slice_bytes(3, 320), state0=PTR, state1=PTR, t=PTR, rms_alpha=0.99,
             rms_eps=1e-5, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-5, stats=PTR, stream=None)
    assert set(over) <= set(ARGS), over
    a.update(over)
    return [a[k] for k in ARGS]


def _refused(needle, **over):
    _, L = _lib()
    assert L.b747_a2c_update_population(*_args(L, **over)) == INVALID, over
    msg = L.b747_last_error()
    assert needle.encode() in msg and NAME.encode() in msg, msg


def test_the_entry_point_is_declared_and_bound_with_matching_names():
    lib, L = _lib()
    assert lib.ABI_VERSION == 15 and int(L.b747_abi_version()) == 15
    assert re.search(r"#define B747_ABI_VERSION 15\b", _header())
    assert NAME in lib.SIGNATURES and hasattr(L, NAME) and getattr(L, NAME).restype is ctypes.c_int32
    m = re.search(r"int32_t " + NAME + r"\(([^;]*)\);", _header())
    assert m
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert tuple(p.split()[-1].lstrip("*") for p in params) == ARGS
    assert len(lib.SIGNATURES[NAME][0]) == len(ARGS) == 25


def test_the_optimizer_column_is_7_in_the_header_and_in_the_binding():
    from b747_rl_ctrl_amd import ppo
    m = re.search(r"#define B747_PPO_HYPER_OPTIMIZER\s+(\d+)\b", _header())
    assert m and int(m.group(1)) == 7 == ppo.A2C_HYPER_COLUMN["optimizer"]
    assert "means Adam" in re.sub(r"\s+\*?\s*", " ", _header())      # any value other than 1 or 2: said in the header
    assert dict(ppo.A2C_HYPER_COLUMN) == {"learning_rate": 0, "ent_coef": 2, "vf_coef": 3, "max_grad_norm": 4,
                                          "gamma": 5, "gae_lambda": 6, "optimizer": 7}
    # PPO's table is what it was
    assert dict(ppo.HYPER_COLUMN) == {"learning_rate": 0, "clip_range": 1, "ent_coef": 2, "vf_coef": 3,
                                      "max_grad_norm": 4, "gamma": 5, "gae_lambda": 6} and ppo.HYPER_COLS == 8


@pytest.mark.parametrize("field", POINTERS)
def test_null_pointers_are_refused_by_name(field):
    _refused(field + " is NULL", **{field: None})


def test_the_sizes_are_refused():
    _, L = _lib()
    num = int(L.b747_policy_num_params(3))
    for n in (0, -2):
        _refused("n_policies", n_policies=n)
    for b in (0, -5):
        _refused("batch", batch=b)
    _refused("batch", batch=1, rows_stride=1, normalize_advantage=1)
    _refused("rows_stride", rows_stride=319)
    _refused("rows_stride", rows_stride=0)
    for od in (0, 4, 6, 9, 11):
        _refused("obs_dim", obs_dim=od)
    for stride in (0, num - 4):
        _refused("policy_stride", policy_stride=stride)
    for ws in (0, -16, _slice_bytes(3, 320) - 1):
        _refused("workspace_bytes", workspace_bytes=ws)


def test_one_slice_and_a_single_row_pass_validation():
    """With one slice of workspace (chunks of one member) and with batch 1, a later wrong argument is what is named"""
    _, L = _lib()
    assert L.b747_a2c_update_population(*_args(L, workspace_bytes=_slice_bytes(3, 320), stats=None)) == INVALID
    assert b"stats is NULL" in L.b747_last_error()
    assert L.b747_a2c_update_population(*_args(L, batch=1, workspace_bytes=_slice_bytes(3, 1), stats=None)) == INVALID
    assert b"stats is NULL" in L.b747_last_error()


@pytest.mark.parametrize("field", ["rms_alpha", "adam_beta1", "adam_beta2"])
@pytest.mark.parametrize("value", [-0.1, 1.0, 1.5, math.nan])
def test_alpha_and_the_betas_outside_the_half_open_unit_interval(field, value):
    _refused(field, **{field: value})


@pytest.mark.parametrize("field", ["rms_eps", "adam_eps"])
@pytest.mark.parametrize("value", [0.0, -1.0, math.inf, math.nan])
def test_eps_values_that_are_not_finite_and_positive(field, value):
    _refused(field, **{field: value})


def test_the_source_is_a_translation_unit_of_its_own():
    from b747_rl_ctrl_amd import build
    assert any(s.endswith("b747_a2c_population.hip") for s in build.SOURCES)
    assert os.path.exists(os.path.join(ROOT, "b747_rl_ctrl_amd", "csrc", "b747_a2c_population.h"))


# --------------------------------------------------------------------------------------------- a2c_hyper_table --
def test_the_table_defaults_come_from_cfg():
    from b747_rl_ctrl_amd.ppo import A2C_OPTIMIZERS, A2CConfig, a2c_hyper_table
    c = A2CConfig.reference(ent_coef=0.01, gamma=0.95)
    t = a2c_hyper_table(c, 3)
    assert t.dtype.is_floating_point and t.element_size() == 8 and tuple(t.shape) == (3, 8)
    row = [c.learning_rate, 0.0, c.ent_coef, c.vf_coef, c.max_grad_norm, c.gamma, c.gae_lambda,
           float(A2C_OPTIMIZERS.index("rmsprop_tf"))]
    assert t.tolist() == [row] * 3
    assert a2c_hyper_table(c, 3, [{}, {}, {}]).tolist() == t.tolist()
    t = a2c_hyper_table(A2CConfig(), 2, [dict(optimizer="adam", vf_coef=0.25), dict(gae_lambda=0.9, max_grad_norm=2.0)])
    assert t[:, 7].tolist() == [0.0, 1.0] and t[:, 3].tolist() == [0.25, 0.5] and t[:, 6].tolist() == [1.0, 0.9]
    assert t[:, 4].tolist() == [0.5, 2.0] and t[:, 1].tolist() == [0.0, 0.0]


def test_the_table_takes_one_source_per_learning_rate():
    from b747_rl_ctrl_amd.ppo import A2CConfig, a2c_hyper_table
    c = A2CConfig()
    assert a2c_hyper_table(c, 2, None, [1e-3, 2e-3])[:, 0].tolist() == [1e-3, 2e-3]
    assert a2c_hyper_table(c, 2, [dict(learning_rate=1e-3), {}])[:, 0].tolist() == [1e-3, c.learning_rate]
    with pytest.raises(ValueError, match="learning_rate"):
        a2c_hyper_table(c, 2, [dict(learning_rate=1e-3), {}], [1e-3, 2e-3])
    with pytest.raises(ValueError, match="one entry per member"):
        a2c_hyper_table(c, 2, None, [1e-3])
    with pytest.raises(ValueError, match="one entry per member"):
        a2c_hyper_table(c, 2, [{}])
    with pytest.raises(ValueError, match="members"):
        a2c_hyper_table(c, 0)


@pytest.mark.parametrize("row,word", [
    (dict(n_steps=8), "n_steps"), (dict(clip_range=0.2), "clip_range"), (dict(rms_eps=1e-5), "rms_eps"),
    (dict(optimizer="sgd"), "optimizer"), (dict(optimizer=1), "optimizer"),
    (dict(gamma=1.5), "gamma"), (dict(gae_lambda=-0.1), "gae_lambda"), (dict(learning_rate=0.0), "learning_rate"),
    (dict(max_grad_norm=-1.0), "max_grad_norm"), (dict(ent_coef=-0.01), "ent_coef"), (dict(vf_coef=math.nan), "vf_coef"),
    (dict(learning_rate=math.inf), "learning_rate"),
])
def test_the_table_refuses_unknown_keys_and_values_outside_their_range(row, word):
    from b747_rl_ctrl_amd.ppo import A2CConfig, a2c_hyper_table
    with pytest.raises(ValueError, match=word):
        a2c_hyper_table(A2CConfig(), 2, [{}, row])
