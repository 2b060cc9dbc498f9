"""A population of policies and PID gain sets scored in ONE launch (b747_eval_population:
BatchControllerEnv.eval_population, evaluate.pack_policies / population_step_tests / pid_sweep_step_tests) against the
path the project already has: one b747_eval_episodes launch per policy / per gain set, the policy in `params` and
the gains in `consts` -- itself held to the step loop, the CPU restatement and the recorded DLL runs by
tests/test_gpu_eval_episodes.py and tests/test_gpu_eval_matrix.py.

FAITHFUL: bit for bit (NaN == NaN, _same): the seven output rows and what the launch leaves in the batch.  FAST: the
population kernels are other instantiations than k_eval_episodes, so their FMA contraction may differ: length, k and
done exact, the metrics at the bars of tests/test_gpu_eval_episodes.py _close (overshoot 1e-3 relative, rise / settling
time within 0.0100001 s, static error 1e-5, quality 1e-6 relative).

Shapes: tk 10 s, sample_time 0.05 (200 env steps, 1,000 DLL steps; the PID baselines fly sample_time = dt: 1,000 env
steps), state0 = [0, 11000, 250, 0, 0, 0] and the callback's four references."""
import ctypes
import math

import numpy as np
import pytest
import torch

from stepinfo_ref import calc_stepinfo
from test_gpu_eval_episodes import REFS, STATE0, TK, ST, R, T, _close, _same

pytestmark = pytest.mark.gpu

ROWS = ("overshoot", "rise_time", "settling_time", "static_error", "itse", "length", "return")
STATE = ("X", "disc", "k", "mem", "obs", "reward", "done", "terminal_obs", "ep_return", "ep_final_return",
         "ep_final_len")
GAINS = (-40.0, -60.0, -90.0)   # a ~ -2, -3, -4.5 obs[1]


def _law(obs_dim, head):
    """_linear_policy of tests/test_gpu_eval_episodes.py with the head's weight free: a = head tanh(tanh(0.05 obs[1]))"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    net = ActorCritic(obs_dim)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        net.pi_net[0].weight[0, 1] = 0.05
        net.pi_net[2].weight[0, 0] = 1.0
        net.action_net.weight[0, 0] = head
    return net


def _env(n, refs, obs="PID_LIKE", mode="DIRECT_CONTROL", variant="fast", ctrl_type=None, sample_time=ST, h=None):
    """the env of run_step_tests_fused: reset at STATE0 with constant commands"""
    from b747_rl_ctrl_amd import BatchControllerEnv, CtrlMode, CtrlType, ObservationType, RewardType
    m, amax = T.MODES[mode]
    ct = CtrlType.MANUAL if ctrl_type is None else ctrl_type
    env = BatchControllerEnv(n, ObservationType(T.OBS[obs]), RewardType.CLASSIC, True, True, ct,
                             CtrlMode(m) if ct == CtrlType.MANUAL else None, reset_ref_mode=None, tk=TK,
                             sample_time=sample_time, action_max=amax, auto_reset=False, variant=variant)
    env.set_state0(torch.tensor(STATE0, dtype=torch.float64))
    if h is None:
        env.set_reference(vartheta=torch.as_tensor(refs, dtype=torch.float64))
    else:
        env.set_reference(h=torch.as_tensor(h, dtype=torch.float64))
    env.reset()
    return env


def _steps(env):
    return int(math.ceil(TK / env.sample_time - 1e-9))


def _score(env):
    """the scored series of run_step_tests_fused: pitch in degrees against the command"""
    return dict(signal="state_vartheta", scale=180 / math.pi, y_base=env.ref[0] * 180 / math.pi)


def _with_quality(ev, vref):
    from b747_rl_ctrl_amd.evaluate import quality
    out = {k: v.cpu() for k, v in ev.items()}
    out["quality"] = quality(ev["itse"], vref, TK).cpu()
    return out


def _assert_same_envs(pop, ev, ix, ref, evr, jx, ctx):
    """envs ix of the population launch (env pop, rows ev) against envs jx of a reference launch: bit for bit"""
    ix, jx = torch.as_tensor(ix, device="cuda"), torch.as_tensor(jx, device="cuda")
    for k in ROWS:
        assert _same(ev[k][ix], evr[k][jx]), (ctx, k)
    for f in STATE:
        a, b = getattr(pop, f), getattr(ref, f)
        a, b = (a[:, ix], b[:, jx]) if f in ("X", "disc") else (a[ix], b[jx])
        assert _same(a.double(), b.double()), (ctx, f)


def _assert_close_envs(pop, ev, ix, ref, evr, jx, ctx):
    """the FAST bars: length, k and done exact, the metrics as _close"""
    ixt, jxt = torch.as_tensor(ix, device="cuda"), torch.as_tensor(jx, device="cuda")
    assert torch.equal(ev["length"][ixt], evr["length"][jxt]), ctx
    assert torch.equal(pop.k[ixt], ref.k[jxt]) and torch.equal(pop.done[ixt], ref.done[jxt]), ctx
    a, b = _with_quality(ev, pop.ref[0]), _with_quality(evr, ref.ref[0])
    a = {k: v[torch.as_tensor(ix)] for k, v in a.items()}
    b = {k: v[torch.as_tensor(jx)] for k, v in b.items()}
    for j in range(len(ix)):
        _close(a, b, j, (ctx, ix[j]))


def _population_against_single_launches(nets, n, obs, mode, variant):
    """P policies in one launch against P eval_episodes launches of 64 envs each; returns the population's rows"""
    from b747_rl_ctrl_amd.evaluate import pack_policies, packed_policy, quality
    od = T.OBS_DIM[obs]
    refs64 = (REFS * 16)[:64]
    refs = (refs64 * len(nets))[:n]
    pop = _env(n, refs, obs, mode, variant)
    ev = pop.eval_population(_steps(pop), pack_policies(nets, od, pop.device), 64, **_score(pop))
    assert bool(pop.done.all()) and int(ev["length"][0]) == 1000
    mq = []
    check = _assert_same_envs if variant == "faithful" else _assert_close_envs
    for p, net in enumerate(nets):
        ref = _env(64, refs64, obs, mode, variant)
        evr = ref.eval_episodes(_steps(ref), packed_policy(net, od, ref.device), **_score(ref))
        live = min(64, n - 64 * p)                      # the last group may be partial
        check(pop, ev, list(range(64 * p, 64 * p + live)), ref, evr, list(range(live)), (obs, mode, variant, n, p))
        mq.append(float(quality(evr["itse"], ref.ref[0], TK)[:4].mean()))
    return ev, mq


@pytest.mark.parametrize("variant", ["faithful", "fast"])
@pytest.mark.parametrize("n", [192, 134])
def test_three_policies_fly_their_own_groups(n, variant):
    nets = [_law(3, g) for g in GAINS]
    ev, mq = _population_against_single_launches(nets, n, "PID_LIKE", "DIRECT_CONTROL", variant)
    print("mean quality per policy:", mq)
    for a in range(3):                                   # the policies must be told apart by what is measured
        for b in range(a + 1, 3):
            assert abs(mq[a] - mq[b]) > 1e-3, (mq, a, b)
    # the policies in reverse order: the groups' results in reverse order (the last group's live envs only)
    rev, _ = _population_against_single_launches(nets[::-1], n, "PID_LIKE", "DIRECT_CONTROL", variant)
    live = n - 128
    for k in ROWS:
        assert _same(rev[k][128:128 + live], ev[k][0:live]), k        # policy 0: group 2 now
        assert _same(rev[k][64:128], ev[k][64:128]), k
        assert _same(rev[k][0:live], ev[k][128:128 + live]), k


@pytest.mark.parametrize("obs,mode,variant", [("SPEED_MODE", "DIRECT_CONTROL", "fast"),
                                              ("SPEED_MODE", "DIRECT_CONTROL", "faithful"),
                                              ("PID_LIKE", "ADD_DIRECT_CONTROL", "fast")])
def test_other_observation_and_control_cases(obs, mode, variant):
    od = T.OBS_DIM[obs]
    nets = [_law(od, GAINS[0]), _law(od, GAINS[2])]
    for n in (128, 70):
        _, mq = _population_against_single_launches(nets, n, obs, mode, variant)
        assert abs(mq[0] - mq[1]) > 1e-3, mq


# ------------------------------------------------------------------------------- gain sweeps --

def _swept_gains(default, count, seed):
    """row 0 the default gains, then each component scaled by a seeded factor in [0.5, 1.5]"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.5, 1.5, size=(count, 4))
    f[0] = 1.0
    return torch.tensor(np.asarray(default)[None] * f, dtype=torch.float64)


def _consts_launch(refs, gains, loop, variant, ctrl_type, h=None):
    """the parent's path: one eval_episodes launch with the gain set in the batch's consts"""
    from b747_rl_ctrl_amd.agent_test import set_pid_coefs
    env = _env(len(h if refs is None else refs), refs, variant=variant, ctrl_type=ctrl_type, sample_time=None, h=h)
    set_pid_coefs(env, [float(g) for g in gains])
    assert (list(env.consts.PID_CS) if loop == "CS" else list(env.consts.PID_SS)) == [float(g) for g in gains]
    kw = _score(env) if loop == "SS" else dict(signal="state_y", scale=1.0, y_base=env.ref[7])
    return env, env.eval_episodes(_steps(env), None, **kw)


def _cpu_pid_episode(vref, gains):
    """_cpu_pid_episode of tests/test_gpu_eval_episodes.py with the SS PID's gains set (neural/agent.py:296-301)"""
    c = R.RefController(1, None, None, None, tk=TK, sample_time=None)
    for j in range(4):
        c.model._pid_ss[j] = float(gains[j])
    e = R.RefControllerEnv(0, 0, True, True, c)
    e.reset({"state0": np.array(STATE0, float), "kind": "const", "ref": vref, "aero_err": None})
    assert [c.model._pid_ss[j] for j in range(4)] == [float(g) for g in gains]
    t, th = [], []

    def rec(m):
        t.append(m.time)
        th.append(float(np.nan_to_num(m.state[4])) * 180 / math.pi)
    done = False
    while not done:
        _, _, done = e.step(np.float32(0.0), rec)
    return calc_stepinfo(th, vref * 180 / math.pi, ts=t), c.quality(), len(th)


@pytest.fixture(scope="module")
def ss_sweep():
    """70 envs, 70 distinct SS gain sets, AUTO, sample_time = dt, no policy: one launch per variant"""
    from b747_rl_ctrl_amd import CtrlType
    from b747_rl_ctrl_amd import _lib
    gains = _swept_gains(list(_lib.default_consts().PID_SS), 70, seed=747)
    assert len({tuple(g.tolist()) for g in gains}) == 70
    refs = (REFS * 18)[:70]
    out = {"gains": gains, "refs": refs}
    for variant in ("faithful", "fast"):
        env = _env(70, refs, variant=variant, ctrl_type=CtrlType.AUTO, sample_time=None)
        ev = env.eval_population(_steps(env), None, pid_ss=gains.cuda(), **_score(env))
        assert bool(env.done.all())
        out[variant] = (env, ev)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("variant", ["faithful", "fast"])
def test_ss_gain_sweep_matches_the_consts_launches(ss_sweep, variant):
    from b747_rl_ctrl_amd import CtrlType
    env, ev = ss_sweep[variant]
    check = _assert_same_envs if variant == "faithful" else _assert_close_envs
    for i in (0, 1, 63, 64, 69):                         # both waves, the first and last lanes, the partial wave's last
        ref, evr = _consts_launch(REFS, ss_sweep["gains"][i], "SS", variant, CtrlType.AUTO)
        assert int(evr["length"][i % 4]) == 1000
        check(env, ev, [i], ref, evr, [i % 4], (variant, i))


def test_ss_gain_sweep_matches_the_cpu_reference(ss_sweep):
    """two swept gain sets against oracle/ref_env.py + calc_stepinfo, at the bars of
    test_pid_baseline_without_a_policy_matches_the_cpu_reference"""
    from b747_rl_ctrl_amd.evaluate import quality
    env, ev = ss_sweep["fast"]
    q = quality(ev["itse"], env.ref[0], TK)
    for i in (5, 66):
        info, qr, n = _cpu_pid_episode(ss_sweep["refs"][i], ss_sweep["gains"][i])
        assert int(ev["length"][i]) == n == 1000
        assert abs(float(ev["overshoot"][i])) == pytest.approx(abs(info["overshoot"]), rel=1e-3)
        for k in ("rise_time", "settling_time"):
            if info[k] is None:
                assert math.isnan(float(ev[k][i])), k
            else:
                assert abs(float(ev[k][i]) - info[k]) <= 0.0100001, (k, float(ev[k][i]), info[k])
        assert float(ev["static_error"][i]) == pytest.approx(info["static_error"], abs=1e-5)
        assert float(q[i]) == pytest.approx(qr, rel=1e-6)


def test_swept_gains_change_the_response(ss_sweep):
    """envs 0, 4, 8, ... fly the same reference under different gains: the sweep must be visible in what is scored"""
    _, ev = ss_sweep["faithful"]
    ov = ev["overshoot"][0::4].abs().cpu()
    assert float((ov.max() - ov.min()) / ov.max()) > 0.01, ov


def test_cs_gain_sweep_matches_the_consts_launches():
    """FULL_AUTO, eight CS gain sets, pid_ss NULL: the altitude series against the altitude command"""
    from b747_rl_ctrl_amd import CtrlType, _lib
    gains = _swept_gains(list(_lib.default_consts().PID_CS), 8, seed=11)
    h = [11000.0 + dh for dh in (50.0, -50.0, 100.0, -100.0)] * 2
    env = _env(8, None, variant="faithful", ctrl_type=CtrlType.FULL_AUTO, sample_time=None, h=h)
    ev = env.eval_population(_steps(env), None, pid_cs=gains.cuda(), signal="state_y", scale=1.0, y_base=env.ref[7])
    for i in range(8):
        ref, evr = _consts_launch(None, gains[i], "CS", "faithful", CtrlType.FULL_AUTO, h=h[:4])
        _assert_same_envs(env, ev, [i], ref, evr, [i % 4], ("cs", i))
    assert len({float(v) for v in ev["itse"][0::4]}) == 2      # two gain sets on one command: two responses


def test_policy_per_group_and_gains_per_env_together():
    """ADD_DIRECT: the policy adds to the SS PID's command.  70 envs, two policies, three gain sets dealt round robin"""
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.agent_test import set_pid_coefs
    from b747_rl_ctrl_amd.evaluate import pack_policies, packed_policy
    nets = [_law(3, GAINS[0]), _law(3, GAINS[2])]
    sets = _swept_gains(list(_lib.default_consts().PID_SS), 3, seed=3)
    refs64 = (REFS * 16)[:64]
    n = 70
    pop = _env(n, (refs64 * 2)[:n], mode="ADD_DIRECT_CONTROL", variant="faithful")
    per_env = sets[torch.arange(n) % 3]
    ev = pop.eval_population(_steps(pop), pack_policies(nets, 3, pop.device), 64, pid_ss=per_env.cuda(), **_score(pop))
    seen = set()
    for p, net in enumerate(nets):
        live = min(64, n - 64 * p)
        for s in range(3):
            ref = _env(live, refs64[:live], mode="ADD_DIRECT_CONTROL", variant="faithful")
            set_pid_coefs(ref, sets[s].tolist())
            evr = ref.eval_episodes(_steps(ref), packed_policy(net, 3, ref.device), **_score(ref))
            jx = [j for j in range(live) if (64 * p + j) % 3 == s]
            _assert_same_envs(pop, ev, [64 * p + j for j in jx], ref, evr, jx, ("both", p, s))
            seen.add(float(evr["itse"][jx[0]]))
    assert len(seen) > 3                                    # policy and gains both reach the dynamics


def test_one_policy_and_no_gains_is_eval_episodes():
    from b747_rl_ctrl_amd.evaluate import pack_policies, packed_policy
    net = _law(3, GAINS[1])
    refs = (REFS * 18)[:70]
    for variant in ("faithful", "fast"):
        pop, ref = _env(70, refs, variant=variant), _env(70, refs, variant=variant)
        ev = pop.eval_population(_steps(pop), pack_policies([net], 3, pop.device), 128, **_score(pop))
        evr = ref.eval_episodes(_steps(ref), packed_policy(net, 3, ref.device), **_score(ref))
        ix = list(range(70))
        (_assert_same_envs if variant == "faithful" else _assert_close_envs)(pop, ev, ix, ref, evr, ix, variant)


# ------------------------------------------------------------------------ the evaluate functions --

def test_population_step_tests_is_run_step_tests_fused_per_policy():
    from b747_rl_ctrl_amd.evaluate import population_step_tests, run_step_tests_fused
    nets = [_law(3, g) for g in GAINS]
    kw = dict(state0=STATE0, tk=TK, sample_time=ST, variant="faithful")
    out = population_step_tests(nets, REFS, **kw)
    assert out["env"].n == 2 * 64 + 4
    for p, net in enumerate(nets):
        one = run_step_tests_fused(net, REFS, **kw)
        for k in ("overshoot", "rise_time", "settling_time", "static_error", "quality", "length", "return", "done"):
            assert out[k].shape == (3, 4) and _same(out[k][p].double(), one[k].double()), (p, k)
        for k in ("mean_quality", "mean_overshoot", "mean_settling_time"):
            # the same four values summed by another reduction kernel: fp64 rounding of the sum (NaN stays NaN)
            assert out[k].shape == (3,) and torch.allclose(out[k][p], one[k], rtol=1e-14, atol=0, equal_nan=True), (p, k)
    assert int(out["best"]) == int(out["mean_quality"].argmax()) == 2


def test_pid_sweep_step_tests_is_the_consts_launch_per_gain_set():
    from b747_rl_ctrl_amd import CtrlMode, CtrlType, _lib
    from b747_rl_ctrl_amd.agent_test import set_pid_coefs
    from b747_rl_ctrl_amd.evaluate import packed_policy, pid_sweep_step_tests, quality
    ss = _swept_gains(list(_lib.default_consts().PID_SS), 3, seed=5)
    out = pid_sweep_step_tests(ss, REFS, "SS", state0=STATE0, tk=TK, variant="faithful")
    assert out["env"].n == 12 and out["env"].ctrl_type == CtrlType.AUTO and out["env"].sample_time == 0.01
    for g in range(3):
        ref, evr = _consts_launch(REFS, ss[g], "SS", "faithful", CtrlType.AUTO)
        for k in ("rise_time", "settling_time", "static_error", "itse"):
            assert out[k].shape == (3, 4) and _same(out[k][g], evr[k]), (g, k)
        assert _same(out["overshoot"][g], evr["overshoot"].abs())
        assert _same(out["quality"][g], quality(evr["itse"], ref.ref[0], TK))
    assert out["mean_quality"].shape == (3,) and int(out["best"]) == int(out["mean_quality"].argmax())
    # a policy on top of the swept SS PID (ADD_DIRECT), one for every env
    net = _law(3, GAINS[0])
    m, amax = T.MODES["ADD_DIRECT_CONTROL"]
    pol = pid_sweep_step_tests(ss, REFS, "SS", policy=net, ctrl_mode=CtrlMode(m), action_max=amax, state0=STATE0, tk=TK,
                               sample_time=ST, variant="faithful")
    for g in range(3):
        ref = _env(4, REFS, mode="ADD_DIRECT_CONTROL", variant="faithful")
        set_pid_coefs(ref, ss[g].tolist())
        evr = ref.eval_episodes(_steps(ref), packed_policy(net, 3, ref.device), **_score(ref))
        assert _same(pol["itse"][g], evr["itse"]) and _same(pol["settling_time"][g], evr["settling_time"]), g
    assert not _same(pol["itse"], out["itse"])
    # the CS loop: altitude commands, the altitude series; no Controller.quality() (see the docstring)
    cs = _swept_gains(list(_lib.default_consts().PID_CS), 2, seed=6)
    h = [11050.0, 10950.0, 11100.0, 10900.0]
    alt = pid_sweep_step_tests(cs, h, "CS", state0=STATE0, tk=TK, variant="faithful")
    assert alt["env"].ctrl_type == CtrlType.FULL_AUTO and "quality" not in alt and "mean_quality" not in alt
    for g in range(2):
        ref, evr = _consts_launch(None, cs[g], "CS", "faithful", CtrlType.FULL_AUTO, h=h)
        for k in ("settling_time", "static_error", "itse"):
            assert _same(alt[k][g], evr[k]), (g, k)
    assert int(alt["best"]) == int(alt["itse"].mean(1).argmin())


# ------------------------------------------------------------------- pack, guards, graph capture --

def test_pack_policies_rows_are_packed_policy():
    from b747_rl_ctrl_amd.evaluate import pack_policies, packed_policy
    dev = torch.device("cuda", torch.cuda.current_device())
    for od in (3, 5):
        torch.manual_seed(od)
        from b747_rl_ctrl_amd.ppo import ActorCritic
        nets = [ActorCritic(od) for _ in range(3)]
        packed = pack_policies(nets, od, dev)
        assert packed.shape[0] == 3 and packed.shape[1] % 4 == 0
        for p, net in enumerate(nets):
            assert torch.equal(packed[p], packed_policy(net, od, dev)), (od, p)
        flat = torch.stack([net.flat_params().detach() for net in nets])
        assert torch.equal(pack_policies(flat, od, dev), packed)          # the [P, n] tensor form


def test_guards_stay_intact_and_a_captured_graph_replays_the_same_bits():
    """the C ABI on views inside poisoned buffers: a longer policy stride whose tail is poison, eval_out and the gain
    rows with poison behind them; then the same call captured in a graph and replayed after a reset"""
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.model import SIG
    L = _lib.lib()
    nets = [_law(3, g) for g in GAINS]
    n, P, poison = 134, 3, -7.25
    num = int(L.b747_policy_num_params(3))
    stride, guard = num + 8, 64
    params = torch.full((P * stride + guard,), poison, dtype=torch.float32, device="cuda")
    rows = params[:P * stride].view(P, stride)
    rows[:, :num] = 0.0
    for p, net in enumerate(nets):
        fp = net.flat_params().detach().cuda()
        rows[p, :fp.numel()] = fp
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.b747_policy_pack_batch(ptr(params), 3, P, stride, stream), "b747_policy_pack_batch")
    assert bool((rows[:, num:] == poison).all()) and bool((params[P * stride:] == poison).all())
    from b747_rl_ctrl_amd.evaluate import packed_policy
    for p, net in enumerate(nets):
        assert torch.equal(rows[p, :num], packed_policy(net, 3, params.device)), p

    env = _env(n, ((REFS * 16)[:64] * P)[:n], variant="faithful")
    gains = torch.full((4 * n + guard,), float(poison), dtype=torch.float64, device="cuda")
    gains[:4 * n].view(4, n).copy_(torch.tensor(list(env.consts.PID_SS), dtype=torch.float64)[:, None].expand(4, n))
    out = torch.full((7 * n + guard,), float(poison), dtype=torch.float64, device="cuda")
    yb = (env.ref[0] * 180 / math.pi).contiguous()

    def call():
        _lib.check(L.b747_eval_population(env._bref, env._cref, env._kref, ptr(params), P, stride, 64, ptr(gains), None,
                                          _steps(env), SIG["state_vartheta"], 180 / math.pi, ptr(yb), 0.05, -1.0, 1.0,
                                          ptr(out), torch.cuda.current_stream().cuda_stream), "b747_eval_population")
    env._batch()
    call()
    torch.cuda.synchronize()
    assert bool((out[7 * n:] == poison).all()) and bool((gains[4 * n:] == poison).all())
    assert bool((params[P * stride:] == poison).all()) and bool((rows[:, num:] == poison).all())
    first = out[:7 * n].clone()
    state = {f: getattr(env, f).clone() for f in STATE}
    assert not bool((first == poison).any()) and bool(env.done.all())

    env.reset()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    for _ in range(2):
        env.reset()
        out.fill_(poison)
        g.replay()
        torch.cuda.synchronize()
        assert _same(out[:7 * n], first) and bool((out[7 * n:] == poison).all())
        for f in STATE:
            assert _same(getattr(env, f).double(), state[f].double()), f
