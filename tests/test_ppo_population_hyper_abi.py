"""b747_ppo_gae_population, b747_ppo_epoch_population_hyper and b747_ppo_epoch_batched_hyper (include/b747.h, additive
under ABI 15): bound, declared, the hyper-parameter table's layout macros, and the argument validation --
no launch, no GPU (as tests/test_ppo_epoch_batched_abi.py: every pointer below is a fake address that a launch would
fault on, so only invalid calls are made; the entry points refuse them before they touch the device)."""
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
GAE_ARGS = ("rew", "val", "done", "last_value", "T", "N", "n_policies", "envs_per_policy", "hyper_dev", "adv", "ret",
            "stream")
POP_ARGS = ("theta", "n_policies", "policy_stride", "obs_dim", "obs", "act", "old_logp", "adv", "ret", "perm", "n_rows",
            "batch_size", "hyper", "workspace", "grad", "m", "v", "t", "beta1", "beta2", "eps", "stats", "stream")
BATCHED_ARGS = ("theta", "n_policies", "policy_stride", "obs_dim", "obs", "act", "old_logp", "adv", "ret", "perm",
                "n_rows", "batch_size", "hyper_dev", "workspace", "workspace_bytes", "m", "v", "t", "beta1", "beta2",
                "eps", "stats", "stream")
ENTRY_POINTS = {"b747_ppo_gae_population": GAE_ARGS, "b747_ppo_epoch_population_hyper": POP_ARGS,
                "b747_ppo_epoch_batched_hyper": BATCHED_ARGS}
COLUMNS = {"B747_PPO_HYPER_COLS": 8, "B747_PPO_HYPER_LR": 0, "B747_PPO_HYPER_CLIP_RANGE": 1,
           "B747_PPO_HYPER_ENT_COEF": 2, "B747_PPO_HYPER_VF_COEF": 3, "B747_PPO_HYPER_MAX_GRAD_NORM": 4,
           "B747_PPO_HYPER_GAMMA": 5, "B747_PPO_HYPER_GAE_LAMBDA": 6}


def _header():
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        return f.read()


def test_the_entry_points_are_bound_and_declared_under_abi_15():
    from b747_rl_ctrl_amd import _lib
    hdr = _header()
    assert _lib.ABI_VERSION == 15 and int(_lib.lib().b747_abi_version()) == 15
    assert re.search(r"#define B747_ABI_VERSION 15\b", hdr)
    for name, args in ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES and re.search(r"int32_t %s\(" % name, hdr), name
        assert getattr(_lib.lib(), name).restype is ctypes.c_int32
        assert len(_lib.SIGNATURES[name][0]) == len(args), name
        decl = re.search(r"int32_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        assert tuple(names) == args, name
    assert len(GAE_ARGS) == 12 and len(POP_ARGS) == 23 and len(BATCHED_ARGS) == 23


def test_the_table_layout_is_in_the_header():
    hdr = _header()
    for name, value in COLUMNS.items():
        m = re.search(r"#define %s\s+(\d+)\b" % name, hdr)
        assert m and int(m.group(1)) == value, name
    assert sorted(v for k, v in COLUMNS.items() if k != "B747_PPO_HYPER_COLS") == list(range(7))   # column 7: reserved


def test_the_binding_knows_the_table_layout():
    from b747_rl_ctrl_amd import ppo
    assert ppo.HYPER_COLS == COLUMNS["B747_PPO_HYPER_COLS"]
    want = {"learning_rate": "LR", "clip_range": "CLIP_RANGE", "ent_coef": "ENT_COEF", "vf_coef": "VF_COEF",
            "max_grad_norm": "MAX_GRAD_NORM", "gamma": "GAMMA", "gae_lambda": "GAE_LAMBDA"}
    assert {k: COLUMNS["B747_PPO_HYPER_" + v] for k, v in want.items()} == dict(ppo.HYPER_COLUMN)


# ------------------------------------------------------------------------------------- b747_ppo_gae_population --
def _gae_args(**over):
    a = dict(rew=P(FAKE), val=P(FAKE), done=P(FAKE), last_value=P(FAKE), T=14, N=192, n_policies=3, envs_per_policy=64,
             hyper_dev=P(FAKE), adv=P(FAKE), ret=P(FAKE), stream=None)
    a.update(over)
    return [a[k] for k in GAE_ARGS]


@pytest.mark.parametrize("over,word", [({f: None}, (f + " is NULL").encode()) for f in
                                       ("rew", "val", "done", "last_value", "hyper_dev", "adv", "ret")] + [
    (dict(T=-1), b"T < 0"), (dict(N=-1), b"N < 0"),
    (dict(n_policies=0), b"n_policies < 1"), (dict(n_policies=-3), b"n_policies < 1"),
    (dict(envs_per_policy=0), b"envs_per_policy"), (dict(envs_per_policy=-64), b"envs_per_policy"),
    (dict(envs_per_policy=96), b"envs_per_policy"), (dict(envs_per_policy=63), b"envs_per_policy"),
    (dict(N=128), b"N (outside"),        # the last member would be empty
    (dict(N=193), b"N (outside"),        # one env more than three members hold
    (dict(N=64, envs_per_policy=128, n_policies=2), b"N (outside"),
])
def test_gae_population_validates_everything_before_the_launch(over, word):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    assert L.b747_ppo_gae_population(*_gae_args(**over)) == INVALID
    err = L.b747_last_error()
    assert word in err and b"b747_ppo_gae_population" in err, err


def test_gae_population_with_no_steps_or_no_envs_launches_nothing():
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    assert L.b747_ppo_gae_population(*_gae_args(T=0)) == 0        # (no GPU here: a launch would have failed)
    assert L.b747_ppo_gae_population(*_gae_args(N=0)) == 0
    assert L.b747_ppo_gae_population(*_gae_args(T=0, N=0)) == 0


# --------------------------------------------------------------------------------------------- the two epochs --
def _formula(od, batch):
    n_wg = min(256, -(-(-(-batch // 32)) // 2))
    n_params = 128 * od + 8579
    return -(-(1024 + 72 * n_wg + 4 * n_params * (n_wg + 1)) // 16) * 16


def _epoch_args(L, names, **over):
    a = dict(theta=P(FAKE), n_policies=3, policy_stride=int(L.b747_policy_num_params(3)), obs_dim=3, obs=P(FAKE),
             act=P(FAKE), old_logp=P(FAKE), adv=P(FAKE), ret=P(FAKE), perm=P(FAKE), n_rows=896, batch_size=256,
             hyper=P(FAKE), hyper_dev=P(FAKE), workspace=P(FAKE), workspace_bytes=3 * _formula(3, 256), grad=P(FAKE),
             m=P(FAKE), v=P(FAKE), t=P(FAKE), beta1=0.9, beta2=0.999, eps=1e-5, stats=P(FAKE), stream=None)
    a.update(over)
    return [a[k] for k in names]


SHARED = [
    (dict(obs_dim=4), b"obs_dim"), (dict(obs_dim=11), b"obs_dim"),
    (dict(n_policies=0), b"n_policies < 1"), (dict(n_policies=-2), b"n_policies < 1"),
    (dict(policy_stride=0), b"policy_stride"), (dict(policy_stride="short"), b"policy_stride"),
    (dict(policy_stride="odd"), b"policy_stride"),
    (dict(n_rows=1), b"n_rows < 2"), (dict(batch_size=1), b"batch_size < 2"),
    (dict(n_rows=1025, batch_size=64), b"n_rows % batch_size == 1"),
]


def _refused(name, names, over, word):
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
    assert getattr(L, name)(*_epoch_args(L, names, **over)) == INVALID
    err = L.b747_last_error()
    assert word in err and name.encode() in err, err


@pytest.mark.parametrize("over,word", [({f: None}, (f + " is NULL").encode()) for f in
                                       ("theta", "obs", "act", "old_logp", "adv", "ret", "perm", "workspace", "grad",
                                        "m", "v", "t", "hyper", "stats")] + SHARED)
def test_epoch_population_hyper_validates_everything_before_the_first_launch(over, word):
    _refused("b747_ppo_epoch_population_hyper", POP_ARGS, over, word)


@pytest.mark.parametrize("over,word", [({f: None}, (f + " is NULL").encode()) for f in
                                       ("theta", "obs", "act", "old_logp", "adv", "ret", "perm", "workspace", "m", "v",
                                        "t", "hyper_dev", "stats")] + SHARED + [
    (dict(workspace_bytes=0), b"workspace_bytes"), (dict(workspace_bytes=-16), b"workspace_bytes"),
    (dict(workspace_bytes="one_short"), b"workspace_bytes"),
])
def test_epoch_batched_hyper_validates_everything_before_the_first_launch(over, word):
    _refused("b747_ppo_epoch_batched_hyper", BATCHED_ARGS, over, word)
