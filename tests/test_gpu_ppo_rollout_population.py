"""b747_ppo_rollout_population (BatchControllerEnv.ppo_rollout_population; csrc/b747_rollout_population.h): P
learners' stochastic rollouts in ONE launch, each group of 64-env waves under its own policy and its own reward
constants, against the single-policy path: one b747_ppo_rollout_lanes launch per member, on a BatchControllerEnv of
that member's envs with env_offset = p * envs_per_policy, the same noise seed and env seed, and set_rew_config with
the member's config.  That path is itself held to the two-launch path and the oracle by
tests/test_gpu_ppo_rollout_lanes.py, whose shapes and bars these are.

Shapes: T = 14, tk 0.3, sample_time 0.05 (6-step episodes: every env is auto-reset at least twice per rollout), two
consecutive rollouts (the second starts mid-episode with fresh noise); n = 134 at 64 envs per policy (three members, the
last wave with 6 live lanes) and n = 192 at 128 (two waves under one policy, a partial last group of one wave).  The
population's policies sit at a stride 8 floats longer than b747_policy_num_params, the reference's at that number.

Bars.  Exact: done_buf, k, episode, mem, flags, ep_final_len, ep_stats[0], ep_stats[2], step_base.  FAITHFUL: every
rollout buffer and env field bit for bit (NaN == NaN) per member slice.  FAST: rtol 1e-5, atol 1e-6 on the float32
buffers, X and disc within 1e-9 of each row's scale, the episode books at 1e-5.  last_val, both variants: the bits of
b747_policy_act's value_out on the population env's own final obs with the member's packed policy.

Reversed members.  The noise and the reset draws are keyed by the global env id, so group g flies other episodes than
group P - 1 - g whatever its policy: "reversed" is held as (a) the reversed population against the single-policy path
built for the reversed assignment, at the same bars, (b) a group that keeps its member (the middle one of three) gives
the forward run's bits, and (c) every group that changes its member gives other actions and rewards."""
import pytest
import torch

from test_gpu_ppo_rollout_lanes import (ENV_BY_MODE, ENV_F32, ENV_OTHER, ENV_STATE, EXACT_ENV, ROLLOUT_F32, SENTINEL, T,
                                        _action_max, _same_bits, _within_row_scale)

pytestmark = pytest.mark.gpu

SEED, ENV_SEED, PAD = 1, 3, 8
BUFS = ROLLOUT_F32 + ("done_buf",)
CONFIGS = [("PID_LIKE", "DIRECT_CONTROL", "CONST"), ("SPEED_MODE", "ADD_DIRECT_CONTROL", "HYBRID"),
           ("PID_LIKE", "ADD_PROC_CONTROL", "OSCILLATING")]
SHAPES = [(134, 64), (192, 128)]
# the members' reward_configs differ in k0, kf and k1 (and from the default 2, 0.1, 2)
REW_CONFIGS = [{"k0": 3.0, "kf": 0.3, "k1": 4}, {"k0": 1.0, "kf": 0.05, "k1": 1}, {"k0": 2.5, "kf": 0.2, "k1": 3}]


def _member_env(n, offset, obs, mode, reset, variant, rew_config=None):
    from b747_rl_ctrl_amd import (BatchControllerEnv, CtrlMode, CtrlType, ObservationType, ResetRefMode, RewardType)
    env = BatchControllerEnv(n, ObservationType[obs], RewardType.CLASSIC, True, True, CtrlType.MANUAL, CtrlMode[mode],
                             reset_ref_mode=ResetRefMode[reset], tk=0.3, sample_time=0.05,
                             action_max=_action_max(CtrlMode[mode]), seed=ENV_SEED, env_offset=offset, variant=variant)
    env.track_episodes()
    if rew_config is not None:
        env.set_rew_config(rew_config)
    return env


def _nets(od, P):
    """policies from different seeds, their means and standard deviations far enough apart to be told apart"""
    from b747_rl_ctrl_amd.ppo import ActorCritic
    nets = []
    for p in range(P):
        torch.manual_seed(10 + p)
        net = ActorCritic(od)
        with torch.no_grad():
            net.action_net.weight.mul_(50.0)
            net.log_std.fill_(-0.5 - 0.25 * p)
        nets.append(net)
    return nets


class _Run:
    """an env, its rollout buffers with the sentinel row T, and its Philox counter"""

    def __init__(self, env):
        self.env, n, od, dev = env, env.n, env.obs_dim, env.device
        full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)
        self.obs_buf, self.act_buf = full(T + 1, n, od), full(T + 1, n, 1)
        self.logp_buf, self.val_buf, self.rew_buf = full(T + 1, n), full(T + 1, n), full(T + 1, n)
        self.done_buf = torch.ones(T + 1, n, dtype=torch.bool, device=dev)
        self.step_base = torch.zeros(1, dtype=torch.int64, device=dev)
        self.last_val_all = full(n + PAD)
        self.last_val = self.last_val_all[:n]

    def lanes(self, flat):
        from b747_rl_ctrl_amd import _lib
        env, p = self.env, lambda x: x.data_ptr()
        b = env._batch()
        b.action = p(env.action)
        _lib.check(_lib.lib().b747_ppo_rollout_lanes(
            env._bref, env._cref, env._kref, p(flat), SEED, p(self.step_base), T, p(self.obs_buf), p(self.act_buf),
            p(self.logp_buf), p(self.val_buf), p(self.rew_buf), p(self.done_buf), -1.0, 1.0,
            torch.cuda.current_stream().cuda_stream), "b747_ppo_rollout_lanes")

    def population(self, flat, epp, rew_pop=None, last_val=True):
        self.env.ppo_rollout_population(T, flat, self.obs_buf, self.act_buf, self.logp_buf, self.val_buf, self.rew_buf,
                                        self.done_buf, seed=SEED, step_base=self.step_base, envs_per_policy=epp,
                                        rew_pop=rew_pop, last_val=self.last_val if last_val else None)

    def sentinels_intact(self):
        for name in ROLLOUT_F32:
            assert bool((getattr(self, name)[T] == SENTINEL).all()), f"{name}: row T was written"
        assert bool(self.done_buf[T].all()), "done_buf: row T was written"
        assert bool((self.last_val_all[self.env.n:] == SENTINEL).all()), "past last_val[N]"


def _wide(packed):
    """the packed policies at a stride PAD floats longer, the tail of every stride a sentinel"""
    P, num = packed.shape
    flat = torch.full((P, num + PAD), SENTINEL, dtype=torch.float32, device=packed.device)
    flat[:, :num].copy_(packed)
    return flat


def _rew_pop(env, configs):
    """[P, 8] rows of rew_constants, in a buffer with PAD sentinel doubles behind them"""
    rows = torch.tensor([env.rew_constants(c) for c in configs], dtype=torch.float64, device=env.device)
    buf = torch.full((rows.numel() + PAD,), SENTINEL, dtype=torch.float64, device=env.device)
    buf[:rows.numel()].copy_(rows.reshape(-1))
    return buf, buf[:rows.numel()].view(-1, 8)


def _of(t, n, sl):
    """member slice of a population tensor: [N, ...] or [rows, N]"""
    return t[sl] if t.shape[0] == n else t[:, sl]


def _compare_member(pop, ref, sl, faithful, what):
    """the population run's envs sl against a single-policy run of those envs"""
    e1, e2, n = pop.env, ref.env, pop.env.n
    assert torch.equal(pop.done_buf[:T, sl], ref.done_buf[:T]), (what, "done_buf")
    for f in EXACT_ENV:
        assert torch.equal(getattr(e1, f)[sl], getattr(e2, f)), (what, f)
    assert torch.equal(e1.ep_stats[0, sl], e2.ep_stats[0]) and torch.equal(e1.ep_stats[2, sl], e2.ep_stats[2]), what
    assert int(pop.step_base) == int(ref.step_base), (what, "step_base")
    by_mode = ENV_BY_MODE.get(e1.ctrl_mode.name, ())
    if faithful:
        for name in ROLLOUT_F32:
            _same_bits(getattr(pop, name)[:T, sl], getattr(ref, name)[:T], f"{what} {name}")
        for f in ENV_F32 + ENV_STATE + ENV_OTHER + by_mode + ("ep_return", "ep_final_return", "ep_stats"):
            _same_bits(_of(getattr(e1, f), n, sl), getattr(e2, f), f"{what} {f}")
        return
    for name in ROLLOUT_F32:
        torch.testing.assert_close(getattr(pop, name)[:T, sl], getattr(ref, name)[:T], rtol=1e-5, atol=1e-6,
                                   msg=lambda m: f"{what} {name}: {m}")
    for f in ENV_F32:
        torch.testing.assert_close(getattr(e1, f)[sl], getattr(e2, f), rtol=1e-5, atol=1e-6,
                                   msg=lambda m: f"{what} {f}: {m}")
    _within_row_scale(e1.X[:, sl], e2.X, f"{what} X")
    _within_row_scale(e1.disc[:, sl], e2.disc, f"{what} disc")
    torch.testing.assert_close(e1.ep_final_return[sl], e2.ep_final_return, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(e1.ep_stats[1, sl], e2.ep_stats[1], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(e1.ep_return[sl], e2.ep_return, rtol=1e-5, atol=1e-5)


def _last_val_is_the_policy_act_value(pop, flat, sl, p):
    """b747_policy_act's value_out on the population env's own final observation with member p's packed policy"""
    from b747_rl_ctrl_amd import _lib
    env, ptr = pop.env, lambda x: x.data_ptr()
    obs = env.obs[sl].contiguous()
    m = obs.shape[0]
    out = [torch.empty(m, dtype=torch.float32, device=env.device) for _ in range(4)]
    _lib.check(_lib.lib().b747_policy_act(ptr(flat[p]), env.obs_dim, m, ptr(obs), None, SEED, None, 0, sl.start, None,
                                          ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), -1.0, 1.0,
                                          torch.cuda.current_stream().cuda_stream), "b747_policy_act")
    _same_bits(pop.last_val[sl], out[2], f"last_val of member {p}")


def _slices(n, epp):
    return [slice(s, min(s + epp, n)) for s in range(0, n, epp)]


def _run_population(n, epp, obs, mode, reset, variant, order):
    """two rollouts of the population with member order[g] in group g, each compared with the single-policy path;
    returns the population run and its clones of the rollout buffers after the second rollout"""
    from b747_rl_ctrl_amd.evaluate import pack_policies, packed_policy
    faithful, sls = variant == "faithful", _slices(n, epp)
    P = len(sls)
    od = 3 if obs == "PID_LIKE" else 5
    nets = _nets(od, P)
    pop = _Run(_member_env(n, 0, obs, mode, reset, variant))
    flat = _wide(pack_policies([nets[m] for m in order], od, pop.env.device))
    rew_all, rew_pop = _rew_pop(pop.env, [REW_CONFIGS[m] for m in order])
    refs = [_Run(_member_env(sl.stop - sl.start, sl.start, obs, mode, reset, variant, REW_CONFIGS[order[g]]))
            for g, sl in enumerate(sls)]
    ref_flat = [packed_policy(nets[order[g]], od, pop.env.device) for g in range(P)]
    for r in range(2):
        pop.population(flat, epp, rew_pop)
        for g in range(P):
            refs[g].lanes(ref_flat[g])
        torch.cuda.synchronize()
        assert int(pop.step_base) == (r + 1) * T, "step_base advances by T per call"
        assert int(pop.done_buf[:T].sum(0).min()) >= 2, "every env is auto-reset at least twice per rollout"
        for g, sl in enumerate(sls):
            _compare_member(pop, refs[g], sl, faithful, f"rollout {r} group {g} (member {order[g]})")
            _last_val_is_the_policy_act_value(pop, flat, sl, g)
        pop.sentinels_intact()
        num = flat.shape[1] - PAD
        assert bool((flat[:, num:] == SENTINEL).all()), "behind a policy's parameters within its stride"
        assert bool((rew_all[P * 8:] == SENTINEL).all()), "behind rew_pop"
    assert int(pop.env.ep_stats[0].min()) >= 4
    return pop, flat, rew_pop


@pytest.mark.parametrize("variant", ["faithful", "fast"])
@pytest.mark.parametrize("n,epp", SHAPES)
@pytest.mark.parametrize("obs,mode,reset", CONFIGS)
def test_members_fly_their_own_policy_and_reward_constants(obs, mode, reset, n, epp, variant):
    sls = _slices(n, epp)
    P = len(sls)
    fwd, flat, rew_pop = _run_population(n, epp, obs, mode, reset, variant, list(range(P)))
    for a in range(P):                                   # the members' reward rows really differ
        for b in range(a + 1, P):
            assert not torch.equal(rew_pop[a], rew_pop[b])
            assert all(float(rew_pop[a, j]) != float(rew_pop[b, j]) for j in (0, 3, 5)), (a, b, rew_pop)
    # ... and reach the reward: the same population under the batch's constants is rewarded otherwise from step 0 on
    # (the same envs, policies and noise: the first action is the same)
    plain = _Run(_member_env(n, 0, obs, mode, reset, variant))
    plain.population(flat, epp, None)
    first = _Run(_member_env(n, 0, obs, mode, reset, variant))
    first.population(flat, epp, rew_pop)
    torch.cuda.synchronize()
    _same_bits(first.act_buf[0], plain.act_buf[0], "the first action does not depend on the reward constants")
    for g, sl in enumerate(sls):
        differ = (first.rew_buf[0, sl] != plain.rew_buf[0, sl]).float().mean()
        assert float(differ) > 0.9, f"group {g}: its reward row changed {float(differ):.2f} of the first rewards"
    # the members in reverse order (module docstring)
    order = list(range(P))[::-1]
    rev, _, _ = _run_population(n, epp, obs, mode, reset, variant, order)
    for g, sl in enumerate(sls):
        if order[g] == g:
            for name in BUFS:
                _same_bits(getattr(rev, name)[:T, sl], getattr(fwd, name)[:T, sl], f"group {g} keeps its member: {name}")
            _same_bits(rev.last_val[sl], fwd.last_val[sl], f"group {g} keeps its member: last_val")
        else:
            assert not torch.equal(rev.act_buf[:T, sl], fwd.act_buf[:T, sl]), f"group {g}: another member, the same actions"
            assert not torch.equal(rev.rew_buf[:T, sl], fwd.rew_buf[:T, sl]), f"group {g}: another member, the same rewards"


@pytest.mark.parametrize("variant", ["faithful", "fast"])
@pytest.mark.parametrize("obs,mode,reset", [("SPEED_MODE", "ADD_DIRECT_CONTROL", "HYBRID"),
                                            ("PID_LIKE", "ADD_PROC_CONTROL", "OSCILLATING")])
def test_one_policy_without_reward_rows_is_the_rollout_lanes_kernel(obs, mode, reset, variant):
    """n_policies = 1, rew_pop = NULL: b747_ppo_rollout_lanes' bits in both variants -- except val_buf for obs_dim 3,
    which that call takes from the batched value pass after the rollout and this one from the head in the step loop:
    FAITHFUL bit for bit, FAST at the float32 bars.  70 envs under one policy at 128 per policy: two waves, the second
    with 6 live lanes."""
    from b747_rl_ctrl_amd.evaluate import packed_policy
    od = 3 if obs == "PID_LIKE" else 5
    net = _nets(od, 1)[0]
    a, b = _Run(_member_env(70, 0, obs, mode, reset, variant)), _Run(_member_env(70, 0, obs, mode, reset, variant))
    flat = packed_policy(net, od, a.env.device)
    for r in range(2):
        a.population(flat.view(1, -1), 128, None)
        b.lanes(flat)
        torch.cuda.synchronize()
        assert int(a.step_base) == int(b.step_base) == (r + 1) * T
        for name in BUFS:
            if name == "val_buf" and od == 3 and variant == "fast":
                torch.testing.assert_close(a.val_buf[:T], b.val_buf[:T], rtol=1e-5, atol=1e-6)
                continue
            _same_bits(getattr(a, name)[:T], getattr(b, name)[:T], f"rollout {r} {name}")
        for f in EXACT_ENV + ENV_F32 + ENV_STATE + ENV_OTHER + ENV_BY_MODE.get(a.env.ctrl_mode.name, ()) + \
                ("ep_return", "ep_final_return", "ep_stats"):
            _same_bits(getattr(a.env, f), getattr(b.env, f), f"rollout {r} {f}")
        a.sentinels_intact()


def test_last_val_is_optional():
    from b747_rl_ctrl_amd.evaluate import pack_policies
    a = _Run(_member_env(134, 0, "PID_LIKE", "DIRECT_CONTROL", "CONST", "fast"))
    b = _Run(_member_env(134, 0, "PID_LIKE", "DIRECT_CONTROL", "CONST", "fast"))
    flat = pack_policies(_nets(3, 3), 3, a.env.device)
    a.population(flat, 64, None, last_val=False)
    b.population(flat, 64, None)
    torch.cuda.synchronize()
    assert bool((a.last_val_all == SENTINEL).all()), "last_val = NULL: nothing is written"
    for name in BUFS:
        _same_bits(getattr(a, name), getattr(b, name), name)
    _same_bits(a.env.X, b.env.X, "X")


def test_a_captured_population_rollout_replays_to_the_bits_of_a_direct_call():
    from b747_rl_ctrl_amd.evaluate import pack_policies
    cfg = ("SPEED_MODE", "ADD_DIRECT_CONTROL", "HYBRID", "fast")
    a, b = _Run(_member_env(134, 0, *cfg)), _Run(_member_env(134, 0, *cfg))
    flat = _wide(pack_policies(_nets(5, 3), 5, a.env.device))
    _, rew_pop = _rew_pop(a.env, REW_CONFIGS)
    s = torch.cuda.Stream(device=a.env.device)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s), torch.no_grad():   # (the capture launches nothing)
        a.population(flat, 64, rew_pop)
    acts = []
    for r in range(2):                                   # one capture, two replays: fresh noise on each
        g.replay()
        b.population(flat, 64, rew_pop)
        torch.cuda.synchronize()
        assert int(a.step_base) == int(b.step_base) == (r + 1) * T
        for name in BUFS:
            _same_bits(getattr(a, name), getattr(b, name), f"replay {r} {name}")
        _same_bits(a.last_val_all, b.last_val_all, f"replay {r} last_val")
        for f in ("X", "disc", "obs", "k", "episode", "ep_return"):
            _same_bits(getattr(a.env, f), getattr(b.env, f), f"replay {r} {f}")
        acts.append(a.act_buf[:T].clone())
    assert not torch.equal(acts[0], acts[1])


def test_refuses_what_the_kernel_does_not_cover():
    from b747_rl_ctrl_amd import _lib
    from b747_rl_ctrl_amd.evaluate import pack_policies
    run = _Run(_member_env(134, 0, "PID_LIKE", "DIRECT_CONTROL", "CONST", "fast"))
    flat = pack_policies(_nets(3, 3), 3, run.env.device)
    with pytest.raises(_lib.B747Error, match="n \\(outside"):
        run.population(flat[:2], 64)
    with pytest.raises(_lib.B747Error, match="envs_per_policy"):
        run.population(flat, 96)
    torch.cuda.synchronize()
    assert int(run.step_base) == 0 and bool((run.act_buf == SENTINEL).all()), "a refused call launches nothing"
