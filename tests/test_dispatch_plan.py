"""Which kernel a call launches and with what workgroup geometry (csrc/b747_dispatch.h): host logic, no GPU.

The public codes (b747_env_kernel on the built library) are pinned against tests/golden/dispatch_parent.json, recorded
from the library of the commit before the launch plans existed (tests/golden/make_dispatch_parent.py).  Geometry and
the model / PPO plans go through a host build of the same header (tests/native/dispatch_check.cpp, compiled here
with plain g++: the header includes no HIP); their expected values are written out by hand from the rules: 64 envs
per workgroup up to 32,768 envs for the per-step and PPO rollout kernels, up to 16,384 for the K-step rollout and the
one-wave model kernel, the K-step model split up to 16,384."""
import ctypes
import functools
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from b747_rl_ctrl_amd import _lib   # noqa: E402

_spec = importlib.util.spec_from_file_location("make_dispatch_parent",
                                               os.path.join(ROOT, "tests", "golden", "make_dispatch_parent.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

GENERIC, DEFC, RECORDING, SPEC_ONE_WAVE, STEP_SPLIT, ROLLOUT_SPLIT = range(6)   # include/b747.h B747_KERNEL_*
M_ONE_WAVE, M_STEP_SPLIT, M_STEPS_SPLIT = range(3)                              # b747_dispatch.h ModelKernel
FAST, FAITHFUL, MIXED = 0, 1, 2
NS = (1, 64, 70, 16384, 16385, 32768, 32769, 65536)


def test_env_kernel_codes_match_the_parent_commit():
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_parent.json")) as f:
        gold = json.load(f)
    assert gold["columns"] == list(G.COLUMNS) + ["kernel"]
    want = {tuple(r[:-1]): r[-1] for r in gold["rows"]}
    prev = _lib.lib().b747_set_specialization(1)
    _lib.lib().b747_set_specialization(prev)
    got = {tuple(r): code for r, code in G.sweep(_lib)}
    assert _lib.lib().b747_set_specialization(prev) == prev                      # the sweep restored the switch
    assert len(want) == 2 * 2 * 3 * 5 * 3 * 2 * 2 and set(got) == set(want)
    assert set(want.values()) == {GENERIC, DEFC, RECORDING, SPEC_ONE_WAVE, STEP_SPLIT, ROLLOUT_SPLIT}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


@functools.lru_cache(maxsize=None)
def _h():
    so = os.path.join(tempfile.mkdtemp(prefix="b747_dispatch_check"), "libdispatch_check.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                    "-o", so,
                    os.path.join(ROOT, "tests", "native", "dispatch_check.cpp")], check=True)
    return ctypes.CDLL(so)


def plan_env(n, variant=FAST, spec=1, n_env_steps=1, n_sub=1, defc=1, sig=0, x_f64=1, cfg=None):
    """(kernel, x_f64, mix, sub, k1, envs_per_wg)"""
    cfg = cfg or G.training_config(_lib, n_sub)
    b = G.env_batch(_lib, n, 3, variant, sig, x_f64)
    out = (ctypes.c_int32 * 6)()
    _h().b747h_plan_env(ctypes.byref(b), ctypes.byref(cfg), defc, spec, n_env_steps, out)
    return tuple(out)


def plan_model(n, variant=FAST, spec=1, n_steps=1, defc=1, x_f64=1):
    """(kernel, x_f64, envs_per_wg)"""
    b = _lib.ModelBatch()
    b.n, b.x_f64, b.variant = n, x_f64, variant
    out = (ctypes.c_int32 * 3)()
    _h().b747h_plan_model(ctypes.byref(b), defc, spec, n_steps, out)
    return tuple(out)


def plan_ppo(n, variant=FAST, n_sub=1, defc=1, sig=0, x_f64=1, obs_dim=3, cfg=None):
    """(covers, (mix, sub, envs_per_wg))"""
    cfg = cfg or G.training_config(_lib, n_sub)
    b = G.env_batch(_lib, n, obs_dim, variant, sig, x_f64)
    out = (ctypes.c_int32 * 3)()
    covers = _h().b747h_plan_ppo_rollout(ctypes.byref(b), ctypes.byref(cfg), defc, out)
    return covers, tuple(out)


@pytest.mark.parametrize("n", NS)
def test_env_plan_geometry(n):
    step_wg = 64 if n <= 32768 else 256
    roll_wg = 64 if n <= 16384 else 256
    for x in (1, 0):
        # one env step of one DLL step: the per-step split kernel; MIXED is the same kernel with MIX
        assert plan_env(n, FAST, x_f64=x) == (STEP_SPLIT, x, 0, 0, 1, step_wg)
        assert plan_env(n, MIXED, x_f64=x) == (STEP_SPLIT, x, 1, 0, 1, step_wg)
        # K steps, or n_sub DLL steps per env step: the rollout split kernel, SUB for n_sub > 1
        assert plan_env(n, FAST, n_env_steps=7, x_f64=x) == (ROLLOUT_SPLIT, x, 0, 0, 0, roll_wg)
        assert plan_env(n, FAST, n_sub=5, x_f64=x) == (ROLLOUT_SPLIT, x, 0, 1, 0, roll_wg)
        assert plan_env(n, MIXED, n_env_steps=7, n_sub=5, x_f64=x) == (ROLLOUT_SPLIT, x, 1, 1, 0, roll_wg)
    # the one-wave kernels: 256 envs per workgroup at every size, no MIX (MIXED runs the FAST kernels), no SUB
    for variant in (FAST, MIXED):
        assert plan_env(n, variant, spec=2) == (SPEC_ONE_WAVE, 1, 0, 0, 1, 256)
        assert plan_env(n, variant, spec=2, n_sub=5) == (SPEC_ONE_WAVE, 1, 0, 0, 0, 256)
        assert plan_env(n, variant, spec=0, n_env_steps=7) == (DEFC, 1, 0, 0, 0, 256)
        assert plan_env(n, variant, defc=0) == (GENERIC, 1, 0, 0, 1, 256)
        assert plan_env(n, variant, sig=1, n_sub=5) == (RECORDING, 1, 0, 0, 0, 256)
    for spec in (0, 1, 2):   # FAITHFUL folds both specialised choices to DEFC
        assert plan_env(n, FAITHFUL, spec=spec) == (DEFC, 1, 0, 0, 1, 256)
        assert plan_env(n, FAITHFUL, spec=spec, n_env_steps=7, x_f64=0) == (DEFC, 0, 0, 0, 0, 256)
    assert plan_env(n, FAITHFUL, defc=0) == (GENERIC, 1, 0, 0, 1, 256)
    assert plan_env(n, FAITHFUL, sig=1) == (RECORDING, 1, 0, 0, 1, 256)
    cfg = G.training_config(_lib, 1)
    cfg.use_limiter = 1      # outside the training configuration: no specialised kernel
    assert plan_env(n, FAST, cfg=cfg) == (DEFC, 1, 0, 0, 1, 256)


@pytest.mark.parametrize("n", NS)
def test_model_plan(n):
    one_wave_wg = 64 if n <= 16384 else 256
    for x in (1, 0):
        for variant in (FAST, MIXED):                      # (MIXED runs FAST on the model API)
            for spec in (1, 2):                            # (2 is treated as 1)
                assert plan_model(n, variant, spec, 1, x_f64=x) == (M_STEP_SPLIT, x, 64)
                assert plan_model(n, variant, spec, 100, x_f64=x) == ((M_STEPS_SPLIT, x, 64) if n <= 16384 else
                                                                      (M_ONE_WAVE, x, 256))
            for n_steps in (1, 100):
                assert plan_model(n, variant, 0, n_steps, x_f64=x) == (M_ONE_WAVE, x, one_wave_wg)
                assert plan_model(n, variant, 1, n_steps, defc=0, x_f64=x) == (M_ONE_WAVE, x, one_wave_wg)
        for spec in (0, 1, 2):
            for n_steps in (1, 100):
                assert plan_model(n, FAITHFUL, spec, n_steps, x_f64=x) == (M_ONE_WAVE, x, one_wave_wg)


@pytest.mark.parametrize("n", NS)
def test_ppo_rollout_geometry(n):
    wg = 64 if n <= 32768 else 256
    assert plan_ppo(n)[1] == (0, 0, wg)
    assert plan_ppo(n, MIXED, n_sub=5)[1] == (1, 1, wg)
    assert plan_ppo(n, FAST, n_sub=5)[1] == (0, 1, wg)


def test_ppo_rollout_predicate():
    assert plan_ppo(64)[0] == 1 and plan_ppo(64, MIXED, n_sub=5)[0] == 1
    assert plan_ppo(70)[0] == 0                            # n % 64
    # every refusal reason on its own
    assert plan_ppo(64, defc=0)[0] == 0
    assert plan_ppo(64, x_f64=0)[0] == 0
    assert plan_ppo(64, FAITHFUL)[0] == 0
    assert plan_ppo(64, obs_dim=5)[0] == 0
    assert plan_ppo(64, sig=1)[0] == 0
    for field, value in (("obs_type", 1), ("reward_type", 1), ("ctrl_type", 2), ("ctrl_mode", 1), ("reset_ref_mode", 1),
                         ("disturbance_mode", -1), ("norm_obs", 0), ("norm_act", 0), ("use_limiter", 1),
                         ("auto_reset", 0), ("aero_fixed", 1)):
        cfg = G.training_config(_lib, 1)
        setattr(cfg, field, value)
        assert plan_ppo(64, cfg=cfg)[0] == 0, field
    cfg = G.training_config(_lib, 1)                       # values that select no code path stay free
    cfg.tk, cfg.seed, cfg.vartheta_max = 5.0, 7, 0.1
    assert plan_ppo(64, cfg=cfg)[0] == 1


def test_is_default_consts():
    f = _h().b747h_is_default
    c = _lib.default_consts()
    assert f(ctypes.byref(c)) == 1
    for field in ("Iz", "P", "S", "c_", "g", "m0"):
        c = _lib.default_consts()
        setattr(c, field, getattr(c, field) * (1 + 2 ** -52))   # one ulp: the test is bitwise
        assert f(ctypes.byref(c)) == 0, field
    for field in ("PID_CS", "PID_SS"):
        for j in range(4):
            c = _lib.default_consts()
            getattr(c, field)[j] += 1.0
            assert f(ctypes.byref(c)) == 0, (field, j)
