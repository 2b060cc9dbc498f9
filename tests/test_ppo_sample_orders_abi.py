"""b747_ppo_sample_orders (include/b747.h, additive under ABI 15): bound, declared, and the argument
validation -- no launch, no GPU (as tests/test_ppo_population_hyper_abi.py: `perm` below is a fake address that a launch
would fault on, so only calls that are refused, or that launch nothing, are made).  PopulationPPO's ValueErrors as far
as they can be reached without a device.  And the GPU tests' reference (tests/sample_orders_ref.py) against a second,
scalar restatement of the Philox block and against what a sample order must be."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INVALID = -1   # -hipErrorInvalidValue
P = ctypes.c_void_p
FAKE = 0x1000
NAME = "b747_ppo_sample_orders"
ARGS = ("perm", "n_policies", "T", "envs_per_policy", "N", "seed", "step_base", "epoch", "stream")


def _args(**over):
    a = dict(perm=P(FAKE), n_policies=3, T=5, envs_per_policy=64, N=192, seed=7, step_base=P(FAKE), epoch=1, stream=None)
    a.update(over)
    return [a[k] for k in ARGS]


def test_the_entry_point_is_bound_and_declared_under_abi_15():
    from b747_rl_ctrl_amd import _lib
    with open(os.path.join(ROOT, "include", "b747.h")) as f:
        hdr = f.read()
    assert _lib.ABI_VERSION == 15 and int(_lib.lib().b747_abi_version()) == 15
    assert re.search(r"#define B747_ABI_VERSION 15\b", hdr)
    assert NAME in _lib.SIGNATURES and getattr(_lib.lib(), NAME).restype is ctypes.c_int32
    argtypes = _lib.SIGNATURES[NAME][0]
    assert len(argtypes) == len(ARGS) == 9
    assert argtypes[5] is ctypes.c_uint64 and argtypes[7] is ctypes.c_uint32 and argtypes[4] is ctypes.c_int64
    decl = re.search(r"int32_t %s\((.*?)\);" % NAME, hdr, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert tuple(names) == ARGS


@pytest.mark.parametrize("over,word", [
    (dict(perm=None), b"perm is NULL"),
    (dict(n_policies=0), b"n_policies < 1"), (dict(n_policies=-2), b"n_policies < 1"),
    (dict(T=-1), b"T < 0"),
    (dict(envs_per_policy=0), b"envs_per_policy"), (dict(envs_per_policy=-64), b"envs_per_policy"),
    (dict(envs_per_policy=96), b"envs_per_policy"), (dict(envs_per_policy=63), b"envs_per_policy"),
    (dict(N=191), b"N ("),                                   # three members of 64 envs need 192
    (dict(N=0), b"N ("),
    (dict(n_policies=2, envs_per_policy=128, N=255), b"N ("),
    (dict(T=257), b"T * envs_per_policy > 16384"),           # 16,448 rows
    (dict(T=129, envs_per_policy=128, n_policies=1), b"T * envs_per_policy > 16384"),
    (dict(T=2 ** 31 - 1), b"T * envs_per_policy > 16384"),    # (the product is taken in 64 bits)
])
def test_every_refusal_comes_before_the_launch_and_names_its_argument(over, word):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    assert getattr(L, NAME)(*_args(**over)) == INVALID
    err = L.b747_last_error()
    assert word in err and NAME.encode() in err, err


def test_no_steps_launch_nothing():
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    assert getattr(L, NAME)(*_args(T=0)) == 0                 # (no GPU here: a launch would have failed)
    assert getattr(L, NAME)(*_args(T=0, step_base=None)) == 0
    assert getattr(L, NAME)(*_args(T=0, N=200)) == 0          # more envs than the members hold: allowed
    assert getattr(L, NAME)(*_args(T=0, perm=None)) == INVALID


# ------------------------------------------------------------------------------------------------ PopulationPPO --
def _fake_env(n):
    """what PopulationPPO's constructor reads before its first device call"""
    import torch
    return types.SimpleNamespace(n=n, obs_dim=3, device=torch.device("cpu"))


def test_population_refuses_an_unknown_sample_order_and_too_many_rows_before_any_device_work():
    from b747_rl_ctrl_amd.ppo import PopulationPPO, PPOConfig
    with pytest.raises(ValueError, match="sample_order='gpu'"):
        PopulationPPO(_fake_env(192), 3, 64, PPOConfig(n_steps=8), sample_order="gpu")
    # 257 steps of 64 envs: 16,448 rows a member -- the C message
    with pytest.raises(ValueError, match=r"b747_ppo_sample_orders: T \* envs_per_policy > 16384"):
        PopulationPPO(_fake_env(192), 3, 64, PPOConfig(n_steps=257), sample_order="device")
    with pytest.raises(ValueError, match=r"b747_ppo_sample_orders: T \* envs_per_policy > 16384"):
        PopulationPPO(_fake_env(256), 2, 128, PPOConfig(n_steps=129), sample_order="device")
    # a partial last member: its rows would lie outside the rollout
    with pytest.raises(ValueError, match=r"b747_ppo_sample_orders: N \("):
        PopulationPPO(_fake_env(190), 3, 64, PPOConfig(n_steps=8), sample_order="device")


def test_the_keywords_exist_with_the_defaults_that_keep_todays_path():
    import inspect
    from b747_rl_ctrl_amd.ppo import PopulationPPO
    assert inspect.signature(PopulationPPO.__init__).parameters["sample_order"].default == "host"
    learn = inspect.signature(PopulationPPO.learn).parameters
    assert learn["use_graph"].default is False and list(learn)[1:] == ["iterations", "n_steps", "minibatch_order",
                                                                       "use_graph"]


# ------------------------------------------------------------------------------------------------ the reference --
def test_the_references_philox_block_is_the_scalar_restatements():
    import sample_orders_ref as R
    assert R.philox4x32_10_scalar(0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)   # Random123's
    assert R.philox4x32_10_scalar(M := (1 << 64) - 1, *[0xFFFFFFFF] * 4) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6,
                                                                             0x6D5451FD)            # known answers
    rng = np.random.default_rng(3)
    for key in (0, M, R.order_key(5, 0), R.order_key((1 << 40) + 5, (1 << 32) + 7)):
        c = rng.integers(0, 1 << 32, size=(4, 64), dtype=np.uint64)
        c[:, 0], c[:, 1] = 0, 0xFFFFFFFF
        got = R.philox4x32_10(key, *c)
        for q in range(64):
            assert tuple(int(w[q]) for w in got) == R.philox4x32_10_scalar(key, *(int(x) for x in c[:, q])), (key, q)


def test_the_key_folds_both_64_bit_values():
    import sample_orders_ref as R
    assert R.order_key(0, 0) == R.TAG and R.order_key(R.TAG, 5) == 0           # (step_base's low word: the counter's)
    assert R.order_key(0, 1 << 32) == R.TAG ^ R.FOLD
    assert R.order_key(0, 3 << 32) == R.TAG ^ ((3 * R.FOLD) & R.M64)
    assert R.order_key(1 << 63, 0) == R.TAG ^ (1 << 63)
    assert R.order_key(-1, 0) == R.TAG ^ R.M64                                  # (a negative seed: its uint64 bits)


@pytest.mark.parametrize("shape", [(1, 1, 64, 64), (3, 5, 64, 192), (2, 17, 64, 200), (2, 256, 64, 128)])
def test_every_reference_row_is_a_permutation_of_the_members_rows(shape):
    import sample_orders_ref as R
    Pn, T, epp, N = shape
    ref = R.reference_perm(Pn, T, epp, N, 11, 7, 1)
    assert ref.shape == (Pn, T * epp) and ref.dtype == np.int64
    for p in range(Pn):
        want = (np.arange(T)[:, None] * N + p * epp + np.arange(epp)[None]).reshape(-1)
        assert np.array_equal(np.sort(ref[p]), want), p
        assert not np.array_equal(ref[p], want), p                  # (shuffled)
        # the order is the stable argsort of the words: ascending, ties by the row number
        u = R.order_words(11, 7, 1, p, T * epp)
        l = R.local_order(11, 7, 1, p, T * epp)
        k = (u[l].astype(object) << 32) | l.astype(object)
        assert all(a < b for a, b in zip(k[:-1], k[1:])), p
    if Pn > 1:
        assert not np.array_equal(ref[0] - 0 * epp, ref[1] - 1 * epp)           # the members' orders differ
