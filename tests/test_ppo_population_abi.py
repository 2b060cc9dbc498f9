"""b747_ppo_rollout_population and b747_ppo_epoch_population (include/b747.h, additive under ABI 15): bound, and their
argument validation -- no launch, no GPU (as tests/test_eval_population_abi.py: the entry points refuse bad arguments
before they touch the device; every pointer below is a fake address that a launch would fault on, so a valid call is
only ever made with T == 0).  And BatchControllerEnv.rew_constants against what set_rew_config writes."""
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
BUFS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf")
EPOCH_ARGS = ("theta", "n_policies", "policy_stride", "obs_dim", "obs", "act", "old_logp", "adv", "ret", "perm", "n_rows",
              "batch_size", "clip_range", "ent_coef", "vf_coef", "workspace", "grad", "m", "v", "t", "max_grad_norm", "lr",
              "beta1", "beta2", "eps", "stats", "stream")


def _setup(obs_type=0, n=128):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    b, cfg = _lib.EnvBatch(), _lib.EnvConfig()
    assert L.b747_env_config_default(ctypes.byref(cfg), obs_type, 0) == 0
    b.n, b.x_f64, b.obs_dim = n, 1, L.b747_env_obs_dim(obs_type)
    for f in _lib._ENV_PTRS:          # never dereferenced: nothing below launches
        setattr(b, f, FAKE)
    b.sig = None                      # (a recording batch is refused)
    return _lib, L, b, cfg


def _call(L, _lib, b, cfg, consts=True, params=P(FAKE), n_policies=2, stride=None, epp=64, rew_pop=None, T=0,
          last_val=None, act=(-1.0, 1.0), **bufs):
    if stride is None:
        stride = int(L.b747_policy_num_params(b.obs_dim)) if b.obs_dim in (3, 5) else 20000
    ptrs = [bufs.get(k, P(FAKE)) for k in BUFS]
    return L.b747_ppo_rollout_population(ctypes.byref(b), ctypes.byref(cfg),
                                         ctypes.byref(_lib.default_consts()) if consts else None, params, n_policies,
                                         stride, epp, rew_pop, 7, P(FAKE), T, *ptrs, last_val, act[0], act[1], None)


def test_the_entry_points_are_bound_under_abi_15():
    from b747_rl_ctrl_amd import _lib
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        hdr = f.read()
    assert _lib.ABI_VERSION == 15 and int(_lib.lib().b747_abi_version()) == 15
    for name in ("b747_ppo_rollout_population", "b747_ppo_epoch_population"):
        assert name in _lib.SIGNATURES and re.search(r"int32_t %s\(" % name, hdr), name
        assert getattr(_lib.lib(), name).restype is ctypes.c_int32
    assert len(_lib.SIGNATURES["b747_ppo_rollout_population"][0]) == 21
    assert len(_lib.SIGNATURES["b747_ppo_epoch_population"][0]) == len(EPOCH_ARGS)


def test_a_library_without_the_new_entry_points_is_reported_as_stale():
    from b747_rl_ctrl_amd import _lib

    class Old:                        # a library of ABI 15 from before the population entry points
        def __getattr__(self, name):
            if name.endswith("_population") and name.startswith("b747_ppo_"):
                raise AttributeError(name)
            return type("F", (), {})()
    with pytest.raises(_lib.B747Error, match="lacks b747_ppo_rollout_population"):
        _lib.bind(Old(), 15)


def test_rollout_population_validates_without_launching():
    _lib, L, b, cfg = _setup()
    assert _call(L, _lib, b, cfg) == 0                                   # 2 policies x 64 envs, T = 0: valid
    assert _call(L, _lib, b, cfg, rew_pop=P(FAKE), last_val=P(FAKE)) == 0
    b.n = 70
    assert _call(L, _lib, b, cfg) == 0                                   # a partial last group
    assert _call(L, _lib, b, cfg, n_policies=1, epp=128) == 0
    _lib5, L5, b5, cfg5 = _setup(obs_type=1)
    assert _call(L5, _lib5, b5, cfg5) == 0                               # SPEED_MODE (obs_dim 5)
    num = int(L.b747_policy_num_params(3))
    assert _call(L, _lib, b, cfg, stride=num + 4) == 0                   # a longer stride is fine


@pytest.mark.parametrize("case,word", [("obs_dim_7", b"obs_dim"), ("fp32_state", b"x_f64"), ("recording", b"sig"),
                                       ("consts", b"consts is NULL"), ("params", b"params is NULL"), ("T", b"T < 0"),
                                       ("act", b"act_lo > act_hi")] + [(k, (k + " is NULL").encode()) for k in BUFS])
def test_rollout_population_refuses_what_rollout_lanes_refuses(case, word):
    _lib, L, b, cfg = _setup(obs_type=4 if case == "obs_dim_7" else 0)
    kw, Ts = {}, (0, 10)
    if case == "obs_dim_7":
        assert b.obs_dim == 7
    elif case == "fp32_state":
        b.x_f64 = 0
    elif case == "recording":
        b.sig = FAKE
    elif case == "consts":
        kw = dict(consts=False)
    elif case == "params":
        kw = dict(params=None)
    elif case == "T":
        Ts = (-1,)
    elif case == "act":
        kw = dict(act=(1.0, -1.0))
    else:
        kw = {case: None}
    for T in Ts:                                    # refused before any launch: a launch on these addresses would fault
        assert _call(L, _lib, b, cfg, T=T, **kw) == INVALID
        err = L.b747_last_error()
        assert word in err and b"b747_ppo_rollout_population" in err, err


@pytest.mark.parametrize("kw,word", [
    (dict(epp=0), b"envs_per_policy"), (dict(epp=-64), b"envs_per_policy"), (dict(epp=96), b"envs_per_policy"),
    (dict(epp=32), b"envs_per_policy"),
    (dict(n_policies=0), b"n_policies"), (dict(n_policies=-1), b"n_policies"),
    (dict(n_policies=1), b"n (outside"),            # 128 envs > 1 * 64
    (dict(n_policies=3), b"n (outside"),            # 128 envs <= 2 * 64: the third policy would fly nothing
    (dict(n_policies=2, epp=128), b"n (outside"),   # 128 envs <= 1 * 128
    (dict(stride=-1), b"policy_stride"), (dict(stride="short"), b"policy_stride"), (dict(stride="odd"), b"policy_stride"),
])
def test_rollout_population_refuses_a_bad_population_and_names_the_field(kw, word):
    _lib, L, b, cfg = _setup()
    num = int(L.b747_policy_num_params(3))
    assert num % 4 == 0
    kw = dict(kw)
    if kw.get("stride") == "short":
        kw["stride"] = num - 4
    elif kw.get("stride") == "odd":
        kw["stride"] = num + 2
    for T in (0, 10):
        assert _call(L, _lib, b, cfg, T=T, **kw) == INVALID
        err = L.b747_last_error()
        assert word in err and b"b747_ppo_rollout_population" in err, err


def _epoch_args(L, **over):
    lr = (ctypes.c_double * 3)(3e-4, 1e-4, 1e-3)
    a = dict(theta=P(FAKE), n_policies=3, policy_stride=int(L.b747_policy_num_params(3)), obs_dim=3, obs=P(FAKE),
             act=P(FAKE), old_logp=P(FAKE), adv=P(FAKE), ret=P(FAKE), perm=P(FAKE), n_rows=896, batch_size=256,
             clip_range=0.2, ent_coef=0.0, vf_coef=0.5, workspace=P(FAKE), grad=P(FAKE), m=P(FAKE), v=P(FAKE), t=P(FAKE),
             max_grad_norm=0.5, lr=lr, beta1=0.9, beta2=0.999, eps=1e-5, stats=P(FAKE), stream=None)
    a.update(over)
    return [a[k] for k in EPOCH_ARGS]


@pytest.mark.parametrize("over,word", [({f: None}, (f + " is NULL").encode()) for f in
                                       ("theta", "obs", "act", "old_logp", "adv", "ret", "perm", "workspace", "grad", "m",
                                        "v", "t", "lr", "stats")] + [
    (dict(obs_dim=4), b"obs_dim"), (dict(obs_dim=11), b"obs_dim"),
    (dict(n_policies=0), b"n_policies < 1"), (dict(n_policies=-2), b"n_policies < 1"),
    (dict(policy_stride=0), b"policy_stride"), (dict(policy_stride="short"), b"policy_stride"),
    (dict(policy_stride="odd"), b"policy_stride"),
    (dict(n_rows=1), b"n_rows < 2"), (dict(batch_size=1), b"batch_size < 2"),
    (dict(n_rows=1025, batch_size=64), b"n_rows % batch_size == 1"),
])
def test_epoch_population_validates_everything_before_the_first_launch(over, word):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    num = int(L.b747_policy_num_params(3))
    over = dict(over)
    if over.get("policy_stride") == "short":
        over["policy_stride"] = num - 4
    elif over.get("policy_stride") == "odd":
        over["policy_stride"] = num + 2
    assert L.b747_ppo_epoch_population(*_epoch_args(L, **over)) == INVALID
    err = L.b747_last_error()
    assert word in err and b"b747_ppo_epoch_population" in err, err


CONFIGS = {"CLASSIC": [{}, {"k0": 3.5, "kf": 0.25, "k1": 5}, {"k1": 1, "k2": 3, "k3": 0.5, "kITSE": 0.7}],
           "PID_LIKE": [{}, {"k": 4.0}], "QUALITY": [{}, {"k": 1}],
           "MINIMAL": [{}, {"rmax": 0.5, "k2": 0.1}], "TF_REFERENCE": [{}, {"overshoot_ref": 3, "tp_ref": 4, "k": 0.3}]}


@pytest.mark.parametrize("reward", sorted(CONFIGS))
def test_rew_constants_is_what_set_rew_config_writes(reward):
    """(no GPU: an env shell with the two fields the table reads, its configuration the library's default)"""
    from b747_rl_ctrl_amd import BatchControllerEnv, RewardType, _lib
    L = _lib.lib()
    for rc in CONFIGS[reward]:
        env = BatchControllerEnv.__new__(BatchControllerEnv)
        env.reward_type, env.cfg = RewardType[reward], _lib.EnvConfig()
        assert L.b747_env_config_default(ctypes.byref(env.cfg), 0, RewardType[reward].value) == 0
        before = [env.cfg.rew[j] for j in range(8)]
        got = env.rew_constants(rc)
        assert len(got) == 8 and all(isinstance(v, float) for v in got)
        assert [env.cfg.rew[j] for j in range(8)] == before, "rew_constants must not change the configuration"
        if not rc:
            assert got == before == env.rew_constants(None)
        env.set_rew_config(rc)
        assert got == [env.cfg.rew[j] for j in range(8)], (reward, rc)
