"""b747_eval_population and b747_policy_pack_batch (include/b747.h, ABI 15): bound, and their argument validation --
no launch, no GPU (as tests/test_eval_episodes_abi.py: the entry points refuse bad arguments before they touch the
device; every pointer below is a fake address that a launch would fault on)."""
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


def _setup(obs_type=0, n=128):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    b, cfg = _lib.EnvBatch(), _lib.EnvConfig()
    assert L.b747_env_config_default(ctypes.byref(cfg), obs_type, 0) == 0
    cfg.auto_reset = 0
    b.n, b.x_f64, b.obs_dim = n, 1, L.b747_env_obs_dim(obs_type)
    for f in _lib._ENV_PTRS:          # never dereferenced: nothing below launches
        setattr(b, f, FAKE)
    return _lib, L, b, cfg


def _call(L, _lib, b, cfg, params=P(FAKE), n_policies=2, stride=None, epp=64, pid_ss=None, pid_cs=None, steps=0,
          sig_row=9, y_base=P(FAKE), out=P(FAKE), act=(-1.0, 1.0)):
    if stride is None:
        stride = int(L.b747_policy_num_params(b.obs_dim)) if b.obs_dim in (3, 5) else 0
    return L.b747_eval_population(ctypes.byref(b), ctypes.byref(cfg), ctypes.byref(_lib.default_consts()), params,
                                  n_policies, stride, epp, pid_ss, pid_cs, steps, sig_row, 180 / 3.141592653589793,
                                  y_base, 0.05, act[0], act[1], out, None)


def test_abi_version_is_15_in_the_header_the_binding_and_the_library():
    from b747_rl_ctrl_amd import _lib
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define B747_ABI_VERSION (\d+)", hdr).group(1)) == 15
    assert _lib.ABI_VERSION == 15 and int(_lib.lib().b747_abi_version()) == 15
    for name in ("b747_eval_population", "b747_policy_pack_batch"):
        assert name in _lib.SIGNATURES and re.search(r"int32_t %s\(" % name, hdr), name
        assert getattr(_lib.lib(), name).restype is ctypes.c_int32


def test_eval_population_validates_without_launching():
    _lib, L, b, cfg = _setup()
    assert _call(L, _lib, b, cfg) == 0                                   # 2 policies x 64 envs, 0 steps: valid
    assert _call(L, _lib, b, cfg, pid_ss=P(FAKE), pid_cs=P(FAKE)) == 0
    b.n = 70
    assert _call(L, _lib, b, cfg) == 0                                   # a partial last group
    assert _call(L, _lib, b, cfg, n_policies=1, epp=128) == 0
    assert _call(L, _lib, b, cfg, params=None, n_policies=0, stride=0, pid_ss=P(FAKE)) == 0   # no policy: a gain sweep
    _lib5, L5, b5, cfg5 = _setup(obs_type=1)
    assert _call(L5, _lib5, b5, cfg5) == 0                               # SPEED_MODE (obs_dim 5)


@pytest.mark.parametrize("case,word", [("auto_reset", b"auto_reset"), ("fp32_state", b"x_f64"), ("obs_dim_7", b"obs_dim"),
                                       ("sig_row", b"sig_row"), ("y_base", b"NULL"), ("eval_out", b"NULL"),
                                       ("steps", b"n_env_steps"), ("act", b"act_lo"), ("action", b"action")])
def test_eval_population_refuses_what_eval_episodes_refuses(case, word):
    _lib, L, b, cfg = _setup(obs_type=4 if case == "obs_dim_7" else 0)
    kw = {}
    if case == "auto_reset":
        cfg.auto_reset = 1
    elif case == "fp32_state":
        b.x_f64 = 0
    elif case == "obs_dim_7":
        assert b.obs_dim == 7
        kw = dict(stride=20000)
    elif case == "sig_row":
        kw = dict(sig_row=31)
    elif case == "y_base":
        kw = dict(y_base=None)
    elif case == "eval_out":
        kw = dict(out=None)
    elif case == "steps":
        kw = dict(steps=-1)
    elif case == "act":
        kw = dict(act=(1.0, -1.0))
    else:
        b.action = None
        kw = dict(params=None, n_policies=0, stride=0)
    for steps in ((kw.pop("steps"),) if "steps" in kw else (0, 10)):
        assert _call(L, _lib, b, cfg, steps=steps, **kw) == INVALID
        err = L.b747_last_error()
        assert word in err and b"b747_eval_population" in err, err
    if case == "obs_dim_7":                                             # the same observation type without a policy is fine
        assert _call(L, _lib, b, cfg, params=None, n_policies=0, stride=0) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(epp=0), b"envs_per_policy"), (dict(epp=-64), b"envs_per_policy"), (dict(epp=96), b"envs_per_policy"),
    (dict(epp=32), b"envs_per_policy"),
    (dict(n_policies=0), b"n_policies"), (dict(n_policies=-1), b"n_policies"),
    (dict(n_policies=1), b"n (outside"),            # 128 envs > 1 * 64
    (dict(n_policies=3), b"n (outside"),            # 128 envs <= 2 * 64: the third policy would fly nothing
    (dict(n_policies=2, epp=128), b"n (outside"),   # 128 envs <= 1 * 128
    (dict(stride=-1), b"policy_stride"), (dict(stride="short"), b"policy_stride"), (dict(stride="odd"), b"policy_stride"),
    (dict(params=None, n_policies=1, stride=0), b"n_policies"), (dict(params=None, n_policies=2), b"n_policies"),
])
def test_eval_population_refuses_a_bad_population_and_names_the_field(kw, word):
    _lib, L, b, cfg = _setup()
    num = int(L.b747_policy_num_params(3))
    assert num % 4 == 0
    kw = dict(kw)
    if kw.get("stride") == "short":
        kw["stride"] = num - 4
    elif kw.get("stride") == "odd":
        kw["stride"] = num + 2
    for steps in (0, 10):                           # refused before any launch: a launch on these addresses would fault
        assert _call(L, _lib, b, cfg, steps=steps, **kw) == INVALID
        assert word in L.b747_last_error(), L.b747_last_error()
    assert _call(L, _lib, b, cfg, stride=num + 4) == 0                   # a longer stride is fine


def test_policy_pack_batch_validates_without_launching():
    _lib, L, b, cfg = _setup()
    num = int(L.b747_policy_num_params(3))
    assert L.b747_policy_pack_batch(P(FAKE), 3, 0, num, None) == 0       # no policy: nothing to launch
    for args, word in (((None, 3, 2, num), b"params"), ((P(FAKE), 0, 2, num), b"obs_dim"),
                       ((P(FAKE), 11, 2, num), b"obs_dim"), ((P(FAKE), 3, -1, num), b"n_policies"),
                       ((P(FAKE), 3, 65536, num), b"n_policies"), ((P(FAKE), 3, 2, num - 4), b"policy_stride"),
                       ((P(FAKE), 3, 2, num + 1), b"policy_stride")):
        assert L.b747_policy_pack_batch(*args, None) == INVALID
        err = L.b747_last_error()
        assert word in err and b"b747_policy_pack_batch" in err, err
