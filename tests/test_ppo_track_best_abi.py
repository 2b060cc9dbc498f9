"""b747_ppo_track_best (include/b747.h, additive under ABI 15): bound, declared, and the argument
validation -- no launch, no GPU (as tests/test_ppo_sample_orders_abi.py: every pointer below is a fake address that a
launch would fault on, so only calls that are refused are made).  ControlTest's and learn's ValueErrors as far as they
can be reached without a device.  And the GPU tests' reference (tests/control_test_ref.py) against a second,
collections.deque-based restatement, its summation order against np.mean for every length up to 128."""
import ctypes
import inspect
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
NAME = "b747_ppo_track_best"
ARGS = ("eval_out", "n_eval", "vref", "tk", "n_members", "envs_per_policy", "n_refs", "window", "repeat", "params",
        "stride", "ring", "count", "last", "window_mean", "best_quality", "best_eval", "best_params", "stream")
POINTERS = ("eval_out", "vref", "params", "ring", "count", "last", "window_mean", "best_quality", "best_eval",
            "best_params")


def _args(**over):
    a = dict(eval_out=P(FAKE), n_eval=132, vref=P(FAKE), tk=20.0, n_members=3, envs_per_policy=64, n_refs=4, window=30,
             repeat=1, params=P(FAKE), stride=8964, ring=P(FAKE), count=P(FAKE), last=P(FAKE), window_mean=P(FAKE),
             best_quality=P(FAKE), best_eval=P(FAKE), best_params=P(FAKE), stream=None)
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
    assert len(argtypes) == len(ARGS) == 19
    assert argtypes[1] is ctypes.c_int64 and argtypes[3] is ctypes.c_double and argtypes[10] is ctypes.c_int64
    assert all(argtypes[i] is ctypes.c_int32 for i in range(4, 9))
    assert all(argtypes[ARGS.index(k)] is ctypes.c_void_p for k in POINTERS + ("stream",))
    decl = re.search(r"int32_t %s\((.*?)\);" % NAME, hdr, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert tuple(names) == ARGS
    # laid out as b747_ppo_sample_orders is: a kernel header and unit of its own, named in the source list
    from b747_rl_ctrl_amd import build
    assert any(s.endswith("b747_ppo_track.hip") for s in build.SOURCES)
    assert any(d.endswith("b747_ppo_track.h") for d in build.DEPS)


@pytest.mark.parametrize("over,word", [(dict([(k, None)]), (k + " is NULL").encode()) for k in POINTERS] + [
    (dict(n_members=0), b"n_members < 1"), (dict(n_members=-1), b"n_members < 1"),
    (dict(envs_per_policy=0), b"envs_per_policy"), (dict(envs_per_policy=-64), b"envs_per_policy"),
    (dict(envs_per_policy=96), b"envs_per_policy"), (dict(envs_per_policy=63), b"envs_per_policy"),
    (dict(n_refs=0), b"n_refs"), (dict(n_refs=65), b"n_refs"), (dict(n_refs=-1), b"n_refs"),
    (dict(n_eval=131), b"n_eval"),                            # two whole groups and four envs need 132
    (dict(n_eval=193), b"n_eval"), (dict(n_eval=0), b"n_eval"),
    (dict(n_members=1, n_eval=3), b"n_eval"), (dict(n_members=1, n_eval=65), b"n_eval"),
    (dict(n_members=2 ** 31 - 1, n_eval=132), b"n_eval"),     # (the product is taken in 64 bits)
    (dict(window=0), b"window"), (dict(window=129), b"window"), (dict(window=-1), b"window"),
    (dict(repeat=0), b"repeat"), (dict(repeat=257), b"repeat"),
    (dict(stride=0), b"stride"), (dict(stride=3), b"stride"), (dict(stride=8966), b"stride"), (dict(stride=-4), b"stride"),
    (dict(tk=0.0), b"tk"), (dict(tk=-1.0), b"tk"), (dict(tk=float("nan")), b"tk"),
])
def test_every_refusal_comes_before_the_launch_and_names_its_argument(over, word):
    from b747_rl_ctrl_amd import _lib
    L = _lib.lib()
    assert getattr(L, NAME)(*_args(**over)) == INVALID
    err = L.b747_last_error()
    assert word in err and NAME.encode() in err, err


# ------------------------------------------------------------------------------------- ControlTest and learn --
def test_control_test_refuses_bad_arguments_before_any_device_work():
    import b747_rl_ctrl_amd
    from b747_rl_ctrl_amd.ppo import ControlTest
    assert b747_rl_ctrl_amd.ControlTest is ControlTest
    sig = inspect.signature(ControlTest.__init__).parameters
    assert list(sig)[1:] == ["learner", "vartheta_ref", "state0", "log_interval", "window_length", "tk", "env_kwargs"]
    assert sig["state0"].default == (0, 11000, 250, 0, 0, 0) and sig["log_interval"].default == 1000
    assert sig["window_length"].default == 30 and sig["tk"].default is None
    with pytest.raises(ValueError, match="window_length=129"):
        ControlTest(None, [0.1], window_length=129)
    with pytest.raises(ValueError, match="window_length=0"):
        ControlTest(None, [0.1], window_length=0)
    with pytest.raises(ValueError, match="log_interval=0"):
        ControlTest(None, [0.1], log_interval=0)
    with pytest.raises(ValueError, match="65 references"):
        ControlTest(None, [0.1] * 65)
    with pytest.raises(ValueError, match="0 references"):
        ControlTest(None, [])
    with pytest.raises(ValueError, match=r"PopulationPPO or a PPO\(fused=True\)"):
        ControlTest(object(), 0.1)


def test_the_pushes_of_an_iteration_are_the_callbacks_multiples_of_the_log_interval():
    from b747_rl_ctrl_amd.ppo import control_test_pushes
    assert control_test_pushes(4, 8, 5) == [1, 2, 1, 2]
    assert control_test_pushes(3, 2048, 1000) == [2, 2, 2]          # main.py: the initial policy is evaluated twice
    assert control_test_pushes(5, 2, 5) == [0, 0, 1, 0, 1]
    assert control_test_pushes(0, 8, 5) == []
    for T, L in ((8, 5), (7, 3), (2048, 1000), (3, 10)):            # n_calls it * T + 1 .. (it + 1) * T
        want = [sum(1 for c in range(it * T + 1, (it + 1) * T + 1) if c % L == 0) for it in range(12)]
        assert control_test_pushes(12, T, L) == want
    assert control_test_pushes(2, 256, 1) == [256, 256]
    with pytest.raises(ValueError, match="257 evaluations in one iteration"):
        control_test_pushes(1, 257, 1)
    with pytest.raises(ValueError, match="log_interval 0"):
        control_test_pushes(1, 8, 0)


def test_learn_refuses_too_many_pushes_and_a_foreign_control_test_before_any_device_work():
    from b747_rl_ctrl_amd.ppo import PPO, PopulationPPO, PPOConfig
    assert inspect.signature(PPO.learn).parameters["control_test"].default is None

    def fake(cls_learn, ct_of):
        me = types.SimpleNamespace(cfg=PPOConfig(n_steps=600), n_members=3, envs_per_member=64, control_test=None)
        me.control_test = ct_of(me)
        return lambda **kw: cls_learn(me, 1, **kw)

    mine = lambda me: types.SimpleNamespace(learner=me, log_interval=2)
    other = lambda me: types.SimpleNamespace(learner=object(), log_interval=2)
    for learn in (PPO.learn, PopulationPPO.learn):
        with pytest.raises(ValueError, match="300 evaluations in one iteration"):
            fake(learn, mine)()
        with pytest.raises(ValueError, match="another learner"):
            fake(learn, other)()
    me = types.SimpleNamespace(cfg=PPOConfig(n_steps=600), control_test=None)
    with pytest.raises(ValueError, match="300 evaluations in one iteration"):
        PPO.learn(me, 1, control_test=types.SimpleNamespace(learner=me, log_interval=2))


# ---------------------------------------------------------------------------------------------- the reference --
def test_the_eight_accumulator_order_is_np_mean_for_every_length_up_to_128():
    import control_test_ref as R
    rng = np.random.default_rng(5)
    for n in range(1, 129):
        for _ in range(20):
            a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).tolist()
            assert R.mean8(a) == np.mean(a), n
        assert R.mean8([0.1] * n) == np.mean([0.1] * n)
    assert np.isnan(R.mean8([1.0, float("nan"), 2.0]))


@pytest.mark.parametrize("W", [1, 3, 5, 30, 128])
def test_the_reference_is_its_deque_restatement(W):
    import control_test_ref as R
    rng = np.random.default_rng(W)
    calls, Pn = 60, 3
    last = rng.uniform(0.0, 1.0, size=(calls, Pn, 3))
    last[:4, 1, 2] = np.nan                       # a member that starts with NaN quality
    last[10, 0, 0] = np.nan
    repeats = [(1, 2, 1, 3)[c % 4] for c in range(calls)]
    a, b = R.track(list(last), repeats, W), R.track_deque(list(last), repeats, W)
    pushes = 0
    for c, (x, y) in enumerate(zip(a, b)):
        pushes += repeats[c]
        for k in ("window_mean", "best_quality", "best_eval"):
            assert R.same(x[k], y[k]), (c, k)
        assert x["count"].tolist() == [pushes] * Pn
        # the window is the last min(pushes, W) pushes, oldest first
        hist = np.concatenate([np.repeat(last[i:i + 1], repeats[i], axis=0) for i in range(c + 1)])[-W:]
        want = np.array([[np.mean(hist[:, p, m].tolist()) for m in range(3)] for p in range(Pn)])
        assert R.same(x["window_mean"], want), c
        # a save is a new best, and nothing else moves it
        before = a[c - 1]["best_quality"] if c else np.zeros(Pn)
        assert ((x["best_quality"] > before) == x["saved"]).all() and (x["best_quality"] >= before).all()
    assert not any(x["saved"][1] for x in a[:4]) and all(x["best_eval"][1] == -1 for x in a[:4])
    # the ring the kernel keeps holds push k in slot k % W
    ring = R.ring(list(last), repeats, W)
    hist = np.concatenate([np.repeat(last[i:i + 1], repeats[i], axis=0) for i in range(calls)])
    for k in range(max(0, len(hist) - W), len(hist)):
        assert R.same(ring[:, :, k % W], hist[k].T)


def test_the_kernel_tests_scenario_saves_where_its_docstring_says():
    """The hand-made inputs of tests/test_gpu_ppo_track_best.py through the reference alone: the margins of every
    decision, and who saves when"""
    import control_test_ref as R
    import test_gpu_ppo_track_best as G
    ev, vref = G._inputs(3)
    sel = np.array([[p * G.EPP + r for r in range(G.NREF)] for p in range(3)])
    last = [R.means([ev[c, 2][sel].tolist(), np.abs(ev[c, 0][sel]).tolist(),
                     R.quality(ev[c, 4][sel], vref[sel], G.TK).tolist()]) for c in range(G.CALLS)]
    repeats = [G.REPEATS[c % 4] for c in range(G.CALLS)]
    for W in (30, 5):
        ref = R.track(last, repeats, W)
        saves = np.array([w["saved"] for w in ref])
        margins = np.array([w["margin"] for w in ref])
        assert np.all(margins[np.isfinite(margins)] > 1e-9)
        assert saves[:, 0].all() and saves[:7, 2].all() and not saves[7:, 2].any()
        assert not saves[:3, 1].any() and saves[:, 1].any() and not saves[:, 1].all()
