"""b747_ppo_epoch_batched_workspace and b747_ppo_epoch_batched (include/b747.h, additive under ABI 15):
bound, declared, the workspace formula, and the argument validation -- no launch, no GPU (as
tests/test_ppo_population_abi.py: every pointer below is a fake address that a launch would fault on, so only invalid
calls are made; the entry point refuses them before it touches the device)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue
P = ctypes.c_void_p
FAKE = 0x1000
ARGS = ("theta", "n_policies", "policy_stride", "obs_dim", "obs", "act", "old_logp", "adv", "ret", "perm", "n_rows",
        "batch_size", "clip_range", "ent_coef", "vf_coef", "workspace", "workspace_bytes", "m", "v", "t", "max_grad_norm",
        "lr_dev", "beta1", "beta2", "eps", "stats", "stream")


def _formula(od, batch):
    n_wg = min(256, -(-(-(-batch // 32)) // 2))
    n_params = 128 * od + 8579
    return -(-(1024 + 72 * n_wg + 4 * n_params * (n_wg + 1)) // 16) * 16


def test_the_entry_points_are_bound_and_declared_under_abi_15():
    from b747_rl_ctrl_amd import _lib
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        hdr = f.read()
    assert _lib.ABI_VERSION == 15 and int(_lib.lib().b747_abi_version()) == 15
    assert re.search(r"#define B747_ABI_VERSION 15\b", hdr)
    for name, ret in (("b747_ppo_epoch_batched_workspace", "int64_t"), ("b747_ppo_epoch_batched", "int32_t")):
        assert name in _lib.SIGNATURES and re.search(r"%s %s\(" % (ret, name), hdr), name
        assert not name.endswith("_population")
    assert _lib.lib().b747_ppo_epoch_batched_workspace.restype is ctypes.c_int64
    assert _lib.lib().b747_ppo_epoch_batched.restype is ctypes.c_int32
    assert len(_lib.SIGNATURES["b747_ppo_epoch_batched_workspace"][0]) == 2
    assert len(_lib.SIGNATURES["b747_ppo_epoch_batched"][0]) == len(ARGS) == 27
    decl = re.search(r"int32_t b747_ppo_epoch_batched\((.*?)\);", hdr, re.S).group(1)
    names = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).split()[-1].lstrip("*") for a in
             re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert tuple(names) == ARGS


@pytest.mark.parametrize("od,batch", [(3, 2), (3, 64), (3, 65), (3, 4096), (3, 16384), (3, 40000), (10, 257)])
def test_the_workspace_is_the_formula(od, batch):
    from b747_rl_ctrl_amd import _lib
    got = int(_lib.lib().b747_ppo_epoch_batched_workspace(od, batch))
    assert got == _formula(od, batch) and got % 16 == 0, (got, _formula(od, batch))


def test_the_workspace_formula_on_known_values():
    """(the formula above against numbers worked out by hand: one workgroup at 64 rows, two at 65, 256 from 16,321)"""
    up = lambda x: (x + 15) // 16 * 16
    assert _formula(3, 64) == up(1024 + 72 + 4 * 8963 * 2) and _formula(3, 2) == _formula(3, 64)
    assert _formula(3, 65) == up(1024 + 144 + 4 * 8963 * 3)
    assert _formula(3, 16384) == _formula(3, 40000) == up(1024 + 72 * 256 + 4 * 8963 * 257)
    assert _formula(10, 257) == up(1024 + 72 * 5 + 4 * 9859 * 6)


def test_the_workspace_refuses_a_bad_obs_dim_and_a_batch_of_one():
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    assert L.b747_ppo_epoch_batched_workspace(4, 256) == INVALID
    err = L.b747_last_error()
    assert b"obs_dim" in err and b"b747_ppo_epoch_batched_workspace" in err, err
    assert L.b747_ppo_epoch_batched_workspace(3, 1) == INVALID
    err = L.b747_last_error()
    assert b"batch_size" in err and b"b747_ppo_epoch_batched_workspace" in err, err


def _args(L, **over):
    a = dict(theta=P(FAKE), n_policies=3, policy_stride=int(L.b747_policy_num_params(3)), obs_dim=3, obs=P(FAKE),
             act=P(FAKE), old_logp=P(FAKE), adv=P(FAKE), ret=P(FAKE), perm=P(FAKE), n_rows=896, batch_size=256,
             clip_range=0.2, ent_coef=0.0, vf_coef=0.5, workspace=P(FAKE), workspace_bytes=3 * _formula(3, 256),
             m=P(FAKE), v=P(FAKE), t=P(FAKE), max_grad_norm=0.5, lr_dev=P(FAKE), beta1=0.9, beta2=0.999, eps=1e-5,
             stats=P(FAKE), stream=None)
    a.update(over)
    return [a[k] for k in ARGS]


@pytest.mark.parametrize("over,word", [({f: None}, (f + " is NULL").encode()) for f in
                                       ("theta", "obs", "act", "old_logp", "adv", "ret", "perm", "workspace", "m", "v",
                                        "t", "lr_dev", "stats")] + [
    (dict(obs_dim=4), b"obs_dim"), (dict(obs_dim=11), b"obs_dim"),
    (dict(n_policies=0), b"n_policies < 1"), (dict(n_policies=-2), b"n_policies < 1"),
    (dict(policy_stride=0), b"policy_stride"), (dict(policy_stride="short"), b"policy_stride"),
    (dict(policy_stride="odd"), b"policy_stride"),
    (dict(n_rows=1), b"n_rows < 2"), (dict(batch_size=1), b"batch_size < 2"),
    (dict(n_rows=1025, batch_size=64), b"n_rows % batch_size == 1"),
    (dict(workspace_bytes=0), b"workspace_bytes"), (dict(workspace_bytes=-16), b"workspace_bytes"),
    (dict(workspace_bytes="one_short"), b"workspace_bytes"),
])
def test_epoch_batched_validates_everything_before_the_first_launch(over, word):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    num = int(L.b747_policy_num_params(3))
    over = dict(over)
    if over.get("policy_stride") == "short":
        over["policy_stride"] = num - 4
    elif over.get("policy_stride") == "odd":
        over["policy_stride"] = num + 2
    if over.get("workspace_bytes") == "one_short":
        over["workspace_bytes"] = _formula(3, 256) - 1
    assert L.b747_ppo_epoch_batched(*_args(L, **over)) == INVALID
    err = L.b747_last_error()
    assert word in err and b"b747_ppo_epoch_batched" in err, err
