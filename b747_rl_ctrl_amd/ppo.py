"""On-GPU PPO rollout over BatchControllerEnv (BASELINE config 5).

The reference trains `PPO('MlpPolicy', env)` from stable-baselines3 with `hp = {}` (the
hyperparams table is keyed by the string 'PPO', neural/setups.py:29, so `PPO in hyperparams` is
False at neural/agent.py:48): SB3 1.4 defaults -- separate pi/vf MLPs [64, 64] with tanh,
orthogonal init, state-independent log_std (init 0), n_steps 2048, gamma 0.99, gae_lambda 0.95,
clip 0.2, ent 0.0, vf 0.5, max_grad_norm 0.5, Adam lr 3e-4, 10 epochs, batch 64.

Here the policy, the rollout buffer and the env all live on the GPU: one rollout step is
policy forward -> Gaussian sample -> clip to the action space -> b747_env_step, with every
tensor preallocated so the whole n_steps rollout can be captured in one HIP graph.  GAE and the
clipped-surrogate update run on device too (batch size scaled to the env count: SB3's batch of
64 is meant for 4 envs).

Data-parallel over ranks (SURVEY 8(e), config 5 on several GPUs): every rank steps its own env
shard (global env ids rank*N + i, so the Philox streams never overlap) and collects its own rollout;
`process_group` makes the ranks start from rank 0's parameters and average their gradients with
ONE all-reduce of the flat gradient bucket (~9k fp32, 36 KB) per minibatch before clipping and the
Adam step -- the only collective, once per minibatch, never on the rollout path.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Callable, Optional, Union

import torch
import torch.distributed as dist
from torch import nn

from .ctrl_env import BatchControllerEnv


class ActorCritic(nn.Module):
    """SB3 MlpPolicy for a 1-D Box action: pi/vf extractors [64, 64] tanh, action_net, value_net,
    log_std parameter; orthogonal init with SB3's gains (sqrt 2 / 0.01 / 1)."""

    def __init__(self, obs_dim: int, act_dim: int = 1, hidden=(64, 64), log_std_init: float = 0.0):
        super().__init__()

        def mlp():
            layers, d = [], obs_dim
            for h in hidden:
                layers += [nn.Linear(d, h), nn.Tanh()]
                d = h
            return nn.Sequential(*layers)
        self.pi_net, self.vf_net = mlp(), mlp()
        self.action_net = nn.Linear(hidden[-1], act_dim)
        self.value_net = nn.Linear(hidden[-1], 1)
        self.log_std = nn.Parameter(torch.full((act_dim,), float(log_std_init)))
        for m, g in ((self.pi_net, math.sqrt(2)), (self.vf_net, math.sqrt(2)), (self.action_net, 0.01),
                     (self.value_net, 1.0)):
            for lin in m.modules():
                if isinstance(lin, nn.Linear):
                    nn.init.orthogonal_(lin.weight, gain=g)
                    nn.init.zeros_(lin.bias)

    def flat_param_list(self):
        """The parameters in the order b747_policy_act reads them (include/b747.h): pi_net layers,
        vf_net layers, action_net, value_net (weight then bias each), log_std."""
        seq = []
        for m in (self.pi_net, self.vf_net):
            for lin in m:
                if isinstance(lin, nn.Linear):
                    seq += [lin.weight, lin.bias]
        seq += [self.action_net.weight, self.action_net.bias, self.value_net.weight, self.value_net.bias,
                self.log_std]
        return seq

    def flat_params(self):
        """flat_param_list() as one vector."""
        return torch.cat([p.detach().reshape(-1) for p in self.flat_param_list()])

    def forward(self, obs):
        mean = self.action_net(self.pi_net(obs))
        value = self.value_net(self.vf_net(obs)).squeeze(-1)
        return mean, value

    def log_prob(self, mean, actions):
        std = self.log_std.exp()
        return (-((actions - mean) ** 2) / (2 * std * std) - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)

    def entropy(self):
        return (0.5 + 0.5 * math.log(2 * math.pi) + self.log_std).sum()


def _world(group) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def broadcast_parameters(module: nn.Module, group=None, src_rank: int = 0):
    """Every rank takes the parameters of rank `src_rank` of `group` (one flat broadcast)."""
    params = [p.data for p in module.parameters()]
    flat = torch.cat([p.reshape(-1) for p in params])
    src = dist.get_global_rank(group, src_rank) if group is not None else src_rank
    dist.broadcast(flat, src=src, group=group)
    off = 0
    for p in params:
        p.copy_(flat[off:off + p.numel()].view_as(p))
        off += p.numel()


def check_env_shards(env, group=None):
    """Data-parallel PPO needs every rank on its OWN env shard of the SAME size: equal counts,
    or the ranks run different numbers of minibatches and the per-minibatch all-reduce hangs; disjoint
    global env ids [env_offset, env_offset + n) under one reset seed, or the Philox reset draws and policy
    noise (both keyed by the global env id) repeat on every rank and the all-reduce silently averages
    duplicate experience.  One all-gather of (n, env_offset, seed) at construction; every rank sees the
    same table, so every rank raises together (no rank is left waiting in a collective)."""
    world = _world(group)
    if world == 1:
        return
    dev = env.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    seed = int(getattr(getattr(env, "cfg", None), "seed", 0)) & ((1 << 64) - 1)
    seed = seed - (1 << 64) if seed >= 1 << 63 else seed    # the uint64 Philox key as int64 (same bits)
    mine = torch.tensor([int(env.n), int(getattr(env, "env_offset", 0)), seed], dtype=torch.int64, device=dev)
    rows = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(rows, mine, group=group)
    rows = [tuple(int(v) for v in r.cpu().tolist()) for r in rows]
    if len({r[0] for r in rows}) != 1:
        raise ValueError(f"data-parallel PPO: env counts differ across ranks {[r[0] for r in rows]} "
                         "(every rank must run the same number of minibatches)")
    for a in range(world):
        for b in range(a + 1, world):
            (n, oa, sa), (_, ob, sb) = rows[a], rows[b]
            if sa == sb and oa < ob + n and ob < oa + n:
                raise ValueError(f"data-parallel PPO: ranks {a} and {b} hold overlapping env ids "
                                 f"[{oa}, {oa + n}) and [{ob}, {ob + n}) under the same seed -- their experience "
                                 "would be identical; give rank r env_offset = r * n")


def allreduce_gradients(params, group=None):
    """Average the gradients of `params` over the ranks of `group` through ONE flat bucket (a single
    all-reduce of ~36 KB for the 64-64 policy instead of one per parameter tensor)."""
    world = _world(group)
    grads = [p.grad for p in params if p.grad is not None]
    if world == 1 or not grads:
        return
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat.div_(world)
    off = 0
    for g in grads:
        g.copy_(flat[off:off + g.numel()].view_as(g))
        off += g.numel()


_p = torch.Tensor.data_ptr      # a tensor's address, as the C ABI takes it


def load_flat(net: ActorCritic, vec: torch.Tensor):
    """Copy the leading entries of the flat vector `vec` (flat_param_list order) into net's parameters"""
    with torch.no_grad():
        off = 0
        for prm in net.flat_param_list():
            prm.copy_(vec[off:off + prm.numel()].view_as(prm))
            off += prm.numel()


def _rollout_buffers(T: int, n: int, od: int, dev):
    """The time-major rollout of T steps of n envs: obs, act, logp, val, rew, done, adv, ret (zeros on dev)"""
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    return z(T, n, od), z(T, n, 1), z(T, n), z(T, n), z(T, n), z(T, n, dt=torch.bool), z(T, n), z(T, n)


def _step_test_kwargs(env: BatchControllerEnv) -> dict:
    """The settings of a step-response test env that flies what `env` trains (evaluate.run_step_tests' keywords)"""
    return dict(observation_type=env.observation_type, reward_type=env.reward_type, ctrl_mode=env.ctrl_mode,
                norm_obs=env.norm_obs, norm_act=env.norm_act, sample_time=env.sample_time, device=env.device,
                action_max=env.action_max, vartheta_max=env.vartheta_max, use_limiter=env.use_limiter,
                variant={0: "fast", 1: "faithful", 2: "mixed"}[env.variant])


def _train_log(mean, last, loss, explained_variance, std) -> dict:
    """train()'s log values by name.  mean: the eight statistics columns averaged over every minibatch; last: approx_kl
    and kl_term_scale, the last epoch's means of columns 4 and 6 -- scalars (PPO) or [P] tensors (PopulationPPO)"""
    return {"entropy_loss": mean[2], "policy_gradient_loss": mean[0], "value_loss": mean[1], "approx_kl": last[0],
            "clip_fraction": mean[3], "loss": loss, "explained_variance": explained_variance, "std": std,
            "pg_term_scale": mean[5], "kl_term_scale": last[1], "policy_loss": mean[0]}


@dataclass
class PPOConfig:
    n_steps: int = 2048
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    learning_rate: float = 3e-4
    n_epochs: int = 10
    batch_size: int = 65536


# The per-member hyper-parameter table of a population (include/b747.h B747_PPO_HYPER_*): [P, 8] float64,
# one 64-byte row per member, column 7 reserved (0).  The keys are PPOConfig's names.
HYPER_COLS = 8
HYPER_COLUMN = {"learning_rate": 0, "clip_range": 1, "ent_coef": 2, "vf_coef": 3, "max_grad_norm": 4, "gamma": 5,
                "gae_lambda": 6}


def _check_hyper_value(key: str, x, where: str) -> float:
    """x as a float if it is a value `key` may take: finite; gamma and gae_lambda in [0, 1]; clip_range, learning_rate
    and max_grad_norm above 0; ent_coef and vf_coef not negative"""
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"{where}: {key} = {x} is not finite")
    if key in ("gamma", "gae_lambda"):
        if not 0.0 <= x <= 1.0:
            raise ValueError(f"{where}: {key} = {x} is outside [0, 1]")
    elif key in ("clip_range", "learning_rate", "max_grad_norm"):
        if not x > 0.0:
            raise ValueError(f"{where}: {key} = {x} is not above 0")
    elif x < 0.0:
        raise ValueError(f"{where}: {key} = {x} is negative")
    return x


# The default exploration rule of PopulationPPO.exploit: key -> (f_lo, f_hi, min, max).  The factors
# 0.8 / 1.2 are the convention of the population-based-training paper (Jaderberg et al., 2017), not a measured choice;
# the bounds are the reference's PPO trial ranges (neural/setups.py, trial_hyperparams).  Keys not named are copied.
PBT_EXPLORE = {"learning_rate": (0.8, 1.2, 1e-5, 1e-3), "ent_coef": (0.8, 1.2, 0.0, 0.01)}
# (PopulationA2C's: the reference's A2C trial ranges)
A2C_PBT_EXPLORE = {"learning_rate": (0.8, 1.2, 1e-5, 1.0), "ent_coef": (0.8, 1.2, 1e-8, 0.1)}


def explore_table(columns: dict, check, explore: dict, where: str) -> list:
    """b747_ppo_exploit's `explore` argument from a dict key -> (f_lo, f_hi, min, max) over the keys of `columns`
    (HYPER_COLUMN or A2C_HYPER_COLUMN): HYPER_COLS rows of four floats, a column that is not named an identity row
    (factors 1, bounds -inf / +inf: an exact copy).  ValueError for an unknown key, for `optimizer` (a kind, not a
    magnitude: it can only be copied), for factors that are not finite with 0 < f_lo <= f_hi, for a bound outside the
    key's own domain (`check`: _check_hyper_value or _check_a2c_hyper_value) and for min > max."""
    rows = [[1.0, 1.0, -math.inf, math.inf] for _ in range(HYPER_COLS)]
    unknown = sorted(set(explore) - set(columns))
    if unknown:
        raise ValueError(f"{where}: explore: unknown key(s) {unknown}; a member's own values are {sorted(columns)}")
    if "optimizer" in explore:
        raise ValueError(f"{where}: explore: optimizer cannot be perturbed (it names a kind; it is copied with the row)")
    for key, spec in explore.items():
        if len(spec) != 4:
            raise ValueError(f"{where}: explore[{key!r}] takes (f_lo, f_hi, min, max)")
        f_lo, f_hi, lo, hi = (float(x) for x in spec)
        if not (math.isfinite(f_lo) and math.isfinite(f_hi) and 0.0 < f_lo <= f_hi):
            raise ValueError(f"{where}: explore[{key!r}]: factors ({f_lo}, {f_hi}) are not finite with 0 < f_lo <= f_hi")
        lo, hi = check(key, lo, f"{where}: explore[{key!r}] min"), check(key, hi, f"{where}: explore[{key!r}] max")
        if lo > hi:
            raise ValueError(f"{where}: explore[{key!r}]: min {lo} > max {hi}")
        rows[columns[key]] = [f_lo, f_hi, lo, hi]
    return rows


class PBT:
    """The settings of a population-based schedule (truncation selection), attached to a population as
    `pop.pbt = PBT(interval)`: learn() then calls pop.exploit(fraction=, explore=, rewards=) before the device work of
    every iteration it > 0 with it % interval == 0, ranking the members by `score`: "transfer_quality" (the attached
    ControlTest's windowed quality, optimize()'s objective; the step is skipped until a first evaluation exists) or
    "mean_reward" (the previous iteration's per-member mean reward as float64; needs no control test).  A plain
    settings object: it holds no device state."""

    SCORES = ("transfer_quality", "mean_reward")

    def __init__(self, interval: int, fraction: float = 0.25, explore=None, rewards: bool = False,
                 score: str = "transfer_quality"):
        if int(interval) != interval or int(interval) < 1:
            raise ValueError(f"PBT: interval={interval!r} (a whole number of iterations, at least 1)")
        if score not in self.SCORES:
            raise ValueError(f"PBT: score={score!r}: one of {list(self.SCORES)}")
        self.interval, self.fraction, self.explore = int(interval), float(fraction), explore
        self.rewards, self.score = bool(rewards), score


def hyper_table(cfg: PPOConfig, n_members: int, hyper=None, learning_rates=None) -> torch.Tensor:
    """The [n_members, 8] float64 CPU table of per-member hyper-parameters (columns HYPER_COLUMN, the last one 0).
    hyper: None or one dict per member with keys among learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm,
    gamma and gae_lambda; a key a member does not name comes from cfg -- the learning rate from learning_rates[p] where
    that list is given (then no dict may name learning_rate: one source per value).  ValueError for an unknown key, a
    list of the wrong length or a value outside its range (_check_hyper_value).  n_steps, batch_size, n_epochs and the
    network are not keys: they change shapes, and stay the population's."""
    P = int(n_members)
    if P < 1:
        raise ValueError(f"hyper_table: {P} members")
    rows = [{}] * P if hyper is None else list(hyper)
    if len(rows) != P or (learning_rates is not None and len(learning_rates) != P):
        raise ValueError("hyper_table: hyper and learning_rates take one entry per member")
    table = torch.zeros(P, HYPER_COLS, dtype=torch.float64)
    for p, row in enumerate(rows):
        unknown = sorted(set(row) - set(HYPER_COLUMN))
        if unknown:
            raise ValueError(f"hyper_table: member {p}: unknown key(s) {unknown}; a member's own values are "
                             f"{sorted(HYPER_COLUMN)} (n_steps, batch_size, n_epochs and the network are shared)")
        if learning_rates is not None and "learning_rate" in row:
            raise ValueError(f"hyper_table: member {p} names learning_rate although learning_rates is given")
        for key, col in HYPER_COLUMN.items():
            if key in row:
                x = row[key]
            elif key == "learning_rate" and learning_rates is not None:
                x = learning_rates[p]
            else:
                x = getattr(cfg, key)
            table[p, col] = _check_hyper_value(key, x, f"hyper_table: member {p}")
    return table


class PPO:
    """Device-resident PPO on a BatchControllerEnv (action space [-1, 1] with norm_act)."""

    def __init__(self, env: BatchControllerEnv, cfg: Optional[PPOConfig] = None, seed: int = 0, fused: bool = True,
                 rollout_kernel: Union[bool, str, None] = None, process_group=None, data_parallel: Optional[bool] = None,
                 fused_update: bool = False, gae_kernel: Optional[bool] = None, epoch_call: Optional[bool] = None):
        """fused=True: one b747_policy_act launch per rollout step (HIP kernel, include/b747.h);
        fused=False: the same policy as torch modules (reference implementation of the math).
        rollout_kernel (fused only; None = wherever it applies): the whole rollout as ONE
        b747_ppo_rollout launch (policy + env step fused, state in registers across steps) for the
        configuration that kernel covers; False keeps two launches per step.  "lanes" (opt-in, fused only): the
        whole rollout as ONE b747_ppo_rollout_lanes launch for any configuration with a PID_LIKE or SPEED_MODE
        observation and fp64 state -- one wave per 64 envs on the generic lane code, the env state in registers
        across the steps; ValueError with the library's message where it does not apply (INTEGRATION.md says
        when to pick it).
        data_parallel (None = whenever torch.distributed is initialised with more than one rank):
        average the gradients over `process_group` (module docstring); every rank must hold an env
        shard of the same size so that all ranks run the same number of minibatches.
        fused_update (needs fused=True; default False = the torch update, SB3-exact): train() runs every minibatch
        step as b747_ppo_grad + b747_ppo_adam (loss, gradient, clip and Adam in HIP kernels on the flat parameter
        vector, include/b747.h) instead of torch autograd and torch.optim.Adam; held to the torch path within
        fp32 summation order (tests/test_gpu_ppo_update.py).  It keeps its own Adam moments and step count
        (upd_m, upd_v, upd_t) and leaves self.opt alone.
        gae_kernel (None = wherever fused=True and the buffers are on the GPU): compute_gae's recurrence as ONE
        b747_ppo_gae launch instead of the torch loop over the steps; the same bits (tests/test_gpu_ppo_gae.py).  True
        raises where it cannot apply.
        epoch_call (None = wherever fused_update=True and not data-parallel): train() runs each epoch's minibatches
        as ONE b747_ppo_epoch call instead of two calls per minibatch from the interpreter; the same launches, the same
        bits (tests/test_gpu_ppo_epoch.py).  True raises otherwise: data-parallel training keeps the two calls, its
        all-reduce sits between them."""
        self.env, self.cfg = env, cfg or PPOConfig()
        self.fused, self.seed = bool(fused), int(seed)
        self.fused_update = bool(fused_update)
        if self.fused_update and not self.fused:
            raise ValueError("fused_update=True needs fused=True (the flat parameter buffer of the HIP policy)")
        dev, n, T, od = env.device, env.n, self.cfg.n_steps, env.obs_dim
        torch.manual_seed(seed)
        self.policy = ActorCritic(od).to(dev)
        self.group = process_group
        self.data_parallel = (_world(process_group) > 1) if data_parallel is None else bool(data_parallel)
        if epoch_call and not self.fused_update:
            raise ValueError("epoch_call=True needs fused_update=True (b747_ppo_epoch runs the fused minibatch update)")
        if epoch_call and self.data_parallel:
            raise ValueError("epoch_call=True is single-rank only: data-parallel training all-reduces the gradient "
                             "between b747_ppo_grad and b747_ppo_adam, which one b747_ppo_epoch call leaves no room for")
        self.epoch_call = (self.fused_update and not self.data_parallel) if epoch_call is None else bool(epoch_call)
        if self.data_parallel:
            check_env_shards(env, process_group)
            broadcast_parameters(self.policy, process_group)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=self.cfg.learning_rate, eps=1e-5)
        lo, hi = env.action_space.low, env.action_space.high
        self.act_lo, self.act_hi = float(lo), float(hi)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        (self.obs_buf, self.act_buf, self.logp_buf, self.val_buf, self.rew_buf, self.done_buf, self.adv_buf,
         self.ret_buf) = _rollout_buffers(T, n, od, dev)
        self.last_obs = z(n, od)
        self._last_obs_from_env = False   # (rollout kernel: last_obs is env.obs, copied when compute_gae reads it)
        self.last_done = z(n, dt=torch.bool)
        self.noise = z(n, 1)
        self._graph = None
        self._graph_steps = 0
        self.control_test = None          # learn()'s default for its control_test keyword
        if self.fused:
            from . import _lib
            self._lib = _lib
            self._L = _lib.lib()
            self.flat = z(int(self._L.b747_policy_num_params(od)))
            self.step_base = torch.zeros(1, dtype=torch.int64, device=dev)   # Philox counter base
            self.sync_params()
        if self.fused_update:
            ws = int(self._L.b747_ppo_update_workspace(od))
            if ws <= 0:
                raise ValueError(f"fused_update does not cover this policy: {self._L.b747_last_error().decode()}")
            self.n_params = sum(p.numel() for p in self.policy.flat_param_list())
            self.upd_m, self.upd_v, self.upd_grad = z(self.n_params), z(self.n_params), z(self.n_params)
            self.upd_t = torch.zeros(1, dtype=torch.int64, device=dev)       # Adam steps taken, advanced on the device
            self.upd_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        gae_ok = self.fused and torch.device(dev).type == "cuda"
        if gae_kernel and not gae_ok:
            raise ValueError("gae_kernel=True needs fused=True and the rollout buffers on the GPU (b747_ppo_gae)")
        self.gae_kernel = gae_ok if gae_kernel is None else bool(gae_kernel)
        self.rollout_kernel = False
        if isinstance(rollout_kernel, str):
            if rollout_kernel != "lanes":
                raise ValueError(f"rollout_kernel={rollout_kernel!r}: None, True, False or \"lanes\"")
            if not self.fused:
                raise ValueError("rollout_kernel=\"lanes\" needs fused=True (b747_ppo_rollout_lanes reads the packed policy)")
            self.rollout_kernel = "lanes"
            if self._ppo_rollout(0) != 0:                 # T = 0: validates the configuration, launches nothing
                raise ValueError(f"b747_ppo_rollout_lanes does not cover this env: {self._L.b747_last_error().decode()}")
        elif self.fused and rollout_kernel is not False:
            ok = self._ppo_rollout(0) == 0                # T = 0: validates the configuration, launches nothing
            if rollout_kernel and not ok:
                raise ValueError(f"b747_ppo_rollout does not cover this env: {self._L.b747_last_error().decode()}")
            self.rollout_kernel = ok

    def sync_params(self):
        """Copy the policy parameters into the flat fp32 buffer the fused kernel reads."""
        if self.fused:
            with torch.no_grad():
                fp = self.policy.flat_params()
                self.flat[:fp.numel()].copy_(fp)
            self._lib.check(self._L.b747_policy_pack(self.flat.data_ptr(), self.env.obs_dim,
                                                     torch.cuda.current_stream().cuda_stream), "b747_policy_pack")

    # --------------------------------------------------------------- rollout --
    @torch.no_grad()
    def _rollout_step(self, t: int, noise: Optional[torch.Tensor] = None):
        """One policy + env step into rollout row t.  noise [n] (optional, on the env's device): the standard
        normal draws to sample with instead of the generator's -- e.g. a recorded run's own action noise
        (tests/tb_training.py replays the reference's SB3 rollouts this way)."""
        if self.fused:
            return self._rollout_step_fused(t, noise)
        obs = self.last_obs
        mean, value = self.policy(obs)
        if noise is None:
            self.noise.normal_()                  # default CUDA generator: graph-capture safe
        else:
            self.noise.copy_(noise.reshape(self.noise.shape))
        action = mean + self.policy.log_std.exp() * self.noise
        self.obs_buf[t].copy_(obs)
        self.act_buf[t].copy_(action)
        self.logp_buf[t].copy_(self.policy.log_prob(mean, action))
        self.val_buf[t].copy_(value)
        clipped = action.clamp(self.act_lo, self.act_hi)          # SB3 clips before env.step
        o, r, d, _ = self.env.step(clipped.view(-1))
        self.rew_buf[t].copy_(r)
        self.done_buf[t].copy_(d)
        self.last_obs.copy_(o)

    def _rollout_step_fused(self, t: int, noise: Optional[torch.Tensor] = None):
        """Two launches per step: the policy reads the env's current obs and writes the rollout
        row + the env's action buffer; the env step writes reward / done straight into the
        rollout buffers (b747_env_rollout with K = 1).  noise [n] fp32 on the device (optional): the
        kernel's standard normal draws instead of its Philox ones (b747_policy_act's noise argument)."""
        env, p = self.env, _p
        stream = torch.cuda.current_stream().cuda_stream
        if noise is not None:
            assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == env.n \
                and noise.device == env.device, "noise: [n] contiguous fp32 on the env's device"
        self._lib.check(self._L.b747_policy_act(
            p(self.flat), env.obs_dim, env.n, p(env.obs), None if noise is None else p(noise), self.seed,
            p(self.step_base), t,
            env.env_offset, p(self.obs_buf[t]), p(self.act_buf[t]), p(self.logp_buf[t]), p(self.val_buf[t]),
            p(env.action), self.act_lo, self.act_hi, stream), "b747_policy_act")
        env.rollout(env.action.view(1, -1), None, self.rew_buf[t], self.done_buf[t])

    def _ppo_rollout(self, T: int) -> int:
        """The rollout kernel's call (b747_ppo_rollout, or b747_ppo_rollout_lanes for rollout_kernel="lanes": the same
        arguments); the library's return code."""
        env, p = self.env, _p
        b = env._batch()
        call = self._L.b747_ppo_rollout
        if self.rollout_kernel == "lanes":
            call = self._L.b747_ppo_rollout_lanes
            b.action = p(env.action)      # the kernel leaves the last clipped action there (env.step may have pointed
                                          # the descriptor at a caller's buffer)
        return call(env._bref, env._cref, env._kref, p(self.flat), self.seed, p(self.step_base), T,
                    p(self.obs_buf), p(self.act_buf), p(self.logp_buf), p(self.val_buf),
                    p(self.rew_buf), p(self.done_buf), self.act_lo, self.act_hi,
                    torch.cuda.current_stream().cuda_stream)

    def _rollout_call_name(self) -> str:
        return "b747_ppo_rollout_lanes" if self.rollout_kernel == "lanes" else "b747_ppo_rollout"

    def _end_rollout(self, T: int):
        if self.fused:
            self.step_base.add_(T)                    # fresh Philox counters for the next rollout
            self.last_obs.copy_(self.env.obs)         # bootstrap observation for GAE

    def _end_kernel_rollout(self):
        # b747_ppo_rollout and b747_ppo_rollout_lanes advance step_base themselves (ABI 10, 14), and the bootstrap observation is the env's, taken
        # when compute_gae needs it: the captured rollout is then its two kernels and nothing else
        self._last_obs_from_env = True

    def _bootstrap_obs(self) -> torch.Tensor:
        if self._last_obs_from_env:
            self.last_obs.copy_(self.env.obs)
            self._last_obs_from_env = False
        return self.last_obs

    def _graph_key(self, T: int):
        """What a captured rollout graph baked in: the step count, the env's C descriptor (rebuilt when buffers are added,
        e.g. track_episodes / record_signals), the configuration and constants, and the kernel specialisation -- a
        change of any of them re-captures instead of replaying stale arguments"""
        from . import _lib
        env, spec = self.env, int(_lib.lib().b747_get_specialization())
        return (T, env._batch(), bytes(env.cfg), bytes(env.consts), spec)   # (the descriptor itself: no id reuse)

    def collect_rollouts(self, n_steps: Optional[int] = None, use_graph: bool = True):
        """n_steps (default cfg.n_steps) policy+env steps for every env, all on device.  With the rollout kernel the
        bootstrap observation stays in env.obs until compute_gae copies it into last_obs (no copy node in the graph)."""
        T = n_steps or self.cfg.n_steps
        assert T <= self.cfg.n_steps
        if self.rollout_kernel:                      # one launch for the whole rollout
            if not use_graph:
                with torch.no_grad():
                    self._lib.check(self._ppo_rollout(T), self._rollout_call_name())
                self._end_kernel_rollout()
                return T
            # ... and with use_graph, that launch and the value pass replayed as one HIP graph: no host work between
            # the call and the GPU (the configuration, seed and buffers are the capture's, as for the two-launch graph
            # below; the value pass advances step_base on the device)
            if self._graph is None or self._graph_steps != self._graph_key(T):
                s = torch.cuda.Stream(device=self.env.device)
                s.wait_stream(torch.cuda.current_stream())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s), torch.no_grad():
                    self._lib.check(self._ppo_rollout(T), self._rollout_call_name())
                self._graph, self._graph_steps = g, self._graph_key(T)
            self._graph.replay()
            self._end_kernel_rollout()
            return T
        if not use_graph:
            for t in range(T):
                self._rollout_step(t)
            self._end_rollout(T)
            return T
        if self._graph is None or self._graph_steps != self._graph_key(T):
            s = torch.cuda.Stream(device=self.env.device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s), torch.no_grad():     # warm up the policy kernels (no env step)
                mean, _ = self.policy(self.last_obs)
                self.policy.log_prob(mean, mean)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for t in range(T):
                    self._rollout_step(t)
                self._end_rollout(T)
            self._graph, self._graph_steps = g, self._graph_key(T)
        self._graph.replay()
        return T

    @torch.no_grad()
    def compute_gae(self, T: Optional[int] = None):
        """Generalized advantage estimation (SB3 RolloutBuffer.compute_returns_and_advantage).  The bootstrap value is
        one torch forward; the recurrence is one b747_ppo_gae launch over the first T rows (gae_kernel) or the torch
        loop below, whose operation order the kernel keeps: both give the same bits."""
        T = T or self.cfg.n_steps
        c = self.cfg
        _, last_value = self.policy(self._bootstrap_obs())
        if self.gae_kernel:
            p, last_value = _p, last_value.contiguous()
            self._lib.check(self._L.b747_ppo_gae(
                p(self.rew_buf), p(self.val_buf), p(self.done_buf), p(last_value), T, self.env.n, c.gamma, c.gae_lambda,
                p(self.adv_buf), p(self.ret_buf), torch.cuda.current_stream().cuda_stream), "b747_ppo_gae")
            return
        gae = torch.zeros_like(last_value)
        for t in reversed(range(T)):
            next_value = last_value if t == T - 1 else self.val_buf[t + 1]
            nonterminal = (~self.done_buf[t]).float()
            delta = self.rew_buf[t] + c.gamma * next_value * nonterminal - self.val_buf[t]
            gae = delta + c.gamma * c.gae_lambda * nonterminal * gae
            self.adv_buf[t] = gae
        self.ret_buf[:T] = self.adv_buf[:T] + self.val_buf[:T]

    def train(self, T: Optional[int] = None, minibatch_order: Optional[Callable[[int, int, int], torch.Tensor]] = None):
        """Clipped-surrogate PPO epochs over the rollout (SB3 1.4 PPO.train).

        minibatch_order(epoch, T, n) -> [T * n] indices into the time-major rollout (row t * n + env) giving
        the epoch's sample order; default torch.randperm.  (SB3 draws np.random.permutation over its env-major
        flattening, RolloutBuffer.get / swap_and_flatten; tests/tb_transfer.py passes that order to replay a
        recorded SB3 update.)
        Returns SB3's train/* log values: entropy_loss, policy_gradient_loss, value_loss and clip_fraction
        (means over every minibatch), approx_kl (mean over the last epoch's minibatches), loss (the last
        minibatch), explained_variance (of the rollout's values against its returns) and std; policy_loss /
        value_loss repeat the means.  Beside them (not SB3 log values): pg_term_scale = mean |A ratio| over every
        minibatch and kl_term_scale = mean (|ratio| + 1 + |log ratio|) over the last epoch's, the magnitude of the
        terms the two cancelling means sum (the float32 rounding scale of policy_gradient_loss and approx_kl, which the
        replay gates of tests/tb_training.py use).  One host synchronisation at the end."""
        T = T or self.cfg.n_steps
        c = self.cfg
        N = T * self.env.n
        views = (self.obs_buf[:T].reshape(N, -1), self.act_buf[:T].reshape(N, -1), self.logp_buf[:T].reshape(N),
                 self.adv_buf[:T].reshape(N), self.ret_buf[:T].reshape(N))
        n_mb = -(-N // c.batch_size)
        # (the fused update writes its eight statistics, the loss last, straight into the row)
        rows = torch.empty(c.n_epochs * n_mb, 8 if self.fused_update else 7, dtype=torch.float32, device=views[0].device)
        loss, k = None, 0
        for epoch in range(c.n_epochs):
            if minibatch_order is None:
                perm = torch.randperm(N, device=views[0].device)
            else:
                perm = torch.as_tensor(minibatch_order(epoch, T, self.env.n), device=views[0].device)
            if self.epoch_call:     # every minibatch of the epoch from one C call, the statistics straight into rows
                loss = self._epoch_fused(perm, N, rows[k:k + n_mb])
                k += n_mb
                continue
            for i in range(0, N, c.batch_size):
                idx = perm[i:i + c.batch_size]
                if self.fused_update:
                    loss = self._minibatch_fused(idx, rows[k])
                else:
                    loss, st = self._minibatch(idx, views)
                    rows[k].copy_(st)
                k += 1
        if self.fused_update:       # the flat vector is the master copy during the epochs: hand it to the modules
            load_flat(self.policy, self.flat)
        self.sync_params()
        with torch.no_grad():
            v, r = self.val_buf[:T].reshape(N), views[4]
            var_r = r.var(unbiased=False)
            ev = 1 - (r - v).var(unbiased=False) / var_r if float(var_r) != 0 else torch.tensor(float("nan"))
            mean = rows.double().mean(0).tolist()
            last = [float(rows[(c.n_epochs - 1) * n_mb:, k].double().mean()) for k in (4, 6)]
            return _train_log(mean, last, float(loss) if loss is not None else float("nan"), float(ev),
                              float(self.policy.log_std.exp().mean()))

    def _minibatch(self, idx, views):
        """One clipped-surrogate step on the rows `idx` of the rollout views -> (loss, [pg, vf, entropy loss,
        clip fraction, approx_kl, mean |A ratio|, mean (|ratio| + 1 + |log ratio|)])."""
        c = self.cfg
        obs, act, old_logp, adv, ret = views
        mean, value = self.policy(obs[idx])
        logp = self.policy.log_prob(mean, act[idx])
        a = adv[idx]
        a = (a - a.mean()) / (a.std() + 1e-8)
        log_ratio = logp - old_logp[idx]
        ratio = torch.exp(log_ratio)
        pg = -torch.min(a * ratio, a * ratio.clamp(1 - c.clip_range, 1 + c.clip_range)).mean()
        vf = ((ret[idx] - value) ** 2).mean()
        ent_loss = -self.policy.entropy()
        loss = pg + c.ent_coef * ent_loss + c.vf_coef * vf
        with torch.no_grad():
            st = torch.stack([pg, vf, ent_loss, ((ratio - 1).abs() > c.clip_range).float().mean(),
                              ((ratio - 1) - log_ratio).mean(), (a * ratio).abs().mean(),
                              (ratio.abs() + 1 + log_ratio.abs()).mean()])
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        if self.data_parallel:
            allreduce_gradients(self.policy.parameters(), self.group)
        nn.utils.clip_grad_norm_(self.policy.parameters(), c.max_grad_norm)
        self.opt.step()
        return loss.detach(), st

    def _minibatch_fused(self, idx, row):
        """_minibatch as two stream-ordered calls on the flat parameter vector self.flat[:n_params] (no host
        synchronisation): b747_ppo_grad gathers the rows `idx` from the time-major rollout buffers and writes the
        gradient and the statistics row [.., loss]; b747_ppo_adam clips and steps.  Data-parallel: one all-reduce of
        the flat gradient between them, its 1 / world folded into the Adam call.  Returns the loss (a view of row)."""
        c, p = self.cfg, _p
        idx = idx.to(torch.int64).contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        assert idx.numel() >= 2, "a minibatch of one row has no advantage standard deviation"
        self._lib.check(self._L.b747_ppo_grad(
            p(self.flat), self.env.obs_dim, p(self.obs_buf), p(self.act_buf), p(self.logp_buf), p(self.adv_buf),
            p(self.ret_buf), p(idx), idx.numel(), c.clip_range, c.ent_coef, c.vf_coef, p(self.upd_ws), p(self.upd_grad),
            p(row), stream), "b747_ppo_grad")
        world = 1
        if self.data_parallel and dist.is_available() and dist.is_initialized():
            world = _world(self.group)
            dist.all_reduce(self.upd_grad, op=dist.ReduceOp.SUM, group=self.group)
        self._lib.check(self._L.b747_ppo_adam(
            p(self.flat), p(self.upd_m), p(self.upd_v), p(self.upd_t), p(self.upd_grad), self.n_params, 1.0 / world,
            c.max_grad_norm, c.learning_rate, 0.9, 0.999, 1e-5, stream), "b747_ppo_adam")
        return row[7]

    def _epoch_fused(self, perm, N, rows):
        """The minibatch loop of one epoch over the sample order `perm` as one b747_ppo_epoch call: per minibatch the
        launches of _minibatch_fused, from a C loop (single rank).  rows [n_mb][8] receives the statistics.  Returns
        the last minibatch's loss (a view of rows)."""
        c, p = self.cfg, _p
        perm = perm.to(torch.int64).contiguous()
        assert perm.numel() == N, "minibatch_order must give every row of the rollout once"
        self._lib.check(self._L.b747_ppo_epoch(
            p(self.flat), self.env.obs_dim, p(self.obs_buf), p(self.act_buf), p(self.logp_buf), p(self.adv_buf),
            p(self.ret_buf), p(perm), N, c.batch_size, c.clip_range, c.ent_coef, c.vf_coef, p(self.upd_ws),
            p(self.upd_grad), p(self.upd_m), p(self.upd_v), p(self.upd_t), c.max_grad_norm, c.learning_rate, 0.9, 0.999,
            1e-5, p(rows), torch.cuda.current_stream().cuda_stream), "b747_ppo_epoch")
        return rows[-1, 7]

    def learn(self, iterations: int, n_steps: Optional[int] = None, control_test=None):
        """`iterations` x (collect_rollouts, compute_gae, train) after an env reset; train()'s values per iteration, with
        mean_reward.  control_test (a ControlTest built for this learner; None = self.control_test, and with that None
        too today's calls, bits and keys): before
        an iteration's device work it flies the step tests with the policy the rollout is about to use, as often as the
        reference's callback would during that rollout (control_test_pushes), and the iteration's entry gains
        transfer_settling_time / transfer_overshoot / transfer_quality, [1] device tensors."""
        T = n_steps or self.cfg.n_steps
        control_test = self.control_test if control_test is None else control_test
        pushes = _control_test_plan(self, control_test, iterations, T)
        self.last_obs.copy_(self.env.reset())
        self._last_obs_from_env = False
        hist = []
        for it in range(iterations):
            if pushes is not None and pushes[it]:
                control_test.evaluate(pushes[it])
            self.collect_rollouts(T)
            self.compute_gae(T)
            hist.append(self.train(T) | {"mean_reward": float(self.rew_buf[:T].mean())})
            if pushes is not None:
                hist[-1].update(control_test.history_entry())
        return hist

    def step_tests(self, vartheta_ref, state0=(0, 11000, 250, 0, 0, 0), tk: Optional[float] = None, **kwargs):
        """The reference's ControlTestCallback.calc_stepinfo (neural/callbacks.py:60-100) for the current policy:
        one closed-loop step-response episode per pitch reference on a fresh test env with this env's observation
        / reward / control settings, all inside ONE kernel launch (evaluate.run_step_tests_fused), so a training
        loop can call it between rollouts without leaving the device.  Returns run_step_tests' metrics."""
        from .evaluate import run_step_tests_fused
        e = self.env
        policy = self if self.fused else self.policy      # self: the packed buffer the rollout kernels read (self.flat)
        kw = _step_test_kwargs(e) | kwargs
        return run_step_tests_fused(policy, vartheta_ref, state0=state0, tk=e.tk if tk is None else tk, **kw)


@dataclass
class A2CConfig:
    """SB3 1.4 A2C's defaults.  optimizer: "rmsprop" (torch.optim.RMSprop(alpha=rms_alpha, eps=rms_eps): SB3's
    use_rms_prop=True), "rmsprop_tf" (SB3's RMSpropTFLike, below) or "adam" (torch.optim.Adam(eps=1e-5), betas 0.9 /
    0.999: SB3's use_rms_prop=False; rms_alpha and rms_eps are not read)."""
    n_steps: int = 5
    gamma: float = 0.99
    gae_lambda: float = 1.0
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    learning_rate: float = 7e-4
    normalize_advantage: bool = False
    optimizer: str = "rmsprop"
    rms_alpha: float = 0.99
    rms_eps: float = 1e-5

    @classmethod
    def reference(cls, **kw) -> "A2CConfig":
        """The reference's own entry, neural/setups.py hyperparams[A2C]: optimizer_class=RMSpropTFLike with
        optimizer_kwargs=dict(eps=1e-9) on the 64-64 tanh nets, everything else SB3's default"""
        return cls(**({"optimizer": "rmsprop_tf", "rms_eps": 1e-9} | kw))


A2C_OPTIMIZERS = ("adam", "rmsprop", "rmsprop_tf")      # by B747_OPT_* value (include/b747.h)


class RMSpropTFLike(torch.optim.Optimizer):
    """SB3's RMSpropTFLike (stable_baselines3/common/sb2_compat/rmsprop_tf_like.py) without momentum, centring or
    weight decay: sq = alpha sq + (1 - alpha) g^2, theta -= lr g / sqrt(sq + eps) -- epsilon inside the square root --
    with sq starting at ONES (TensorFlow's initial accumulator)."""

    def __init__(self, params, lr: float = 7e-4, alpha: float = 0.99, eps: float = 1e-5):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for prm in group["params"]:
                if prm.grad is None:
                    continue
                st = self.state[prm]
                if not st:
                    st["step"], st["square_avg"] = 0, torch.ones_like(prm)
                st["step"] += 1
                sq = st["square_avg"]
                sq.mul_(group["alpha"]).addcmul_(prm.grad, prm.grad, value=1 - group["alpha"])
                prm.addcdiv_(prm.grad, sq.add(group["eps"]).sqrt_(), value=-group["lr"])


class A2C(PPO):
    """Device-resident A2C on a BatchControllerEnv (SB3 1.4 A2C): PPO's policy, buffers, rollout kernels,
    GAE, step tests and data-parallel set-up, with ONE gradient step per rollout over all its n_steps * n rows.

    fused_update=False (default; the reference math): torch autograd, clip_grad_norm_ and self.opt, the optimiser
    cfg.optimizer names.  fused_update=True: one b747_a2c_update call on self.flat (include/b747.h) -- the loss and
    gradient kernel, then k_ppo_rmsprop or k_ppo_adam; the optimiser state is upd_sq (ones for "rmsprop_tf") or upd_m /
    upd_v, with the step count upd_t, and self.opt is left alone.  Data-parallel training keeps two calls (b747_a2c_grad,
    then the optimiser's with grad_scale 1 / world), the all-reduce of the flat gradient between them.  Either path
    leaves its statistics row in upd_stats [8] (b747_a2c_grad's layout)."""

    def __init__(self, env: BatchControllerEnv, cfg: Optional[A2CConfig] = None, seed: int = 0, fused: bool = True,
                 rollout_kernel: Union[bool, str, None] = None, process_group=None, data_parallel: Optional[bool] = None,
                 fused_update: bool = False, gae_kernel: Optional[bool] = None):
        cfg = cfg or A2CConfig()
        if cfg.optimizer not in A2C_OPTIMIZERS:
            raise ValueError(f"A2CConfig.optimizer={cfg.optimizer!r}: \"rmsprop\", \"rmsprop_tf\" or \"adam\"")
        super().__init__(env, cfg, seed=seed, fused=fused, rollout_kernel=rollout_kernel, process_group=process_group,
                         data_parallel=data_parallel, fused_update=fused_update, gae_kernel=gae_kernel)
        self.epoch_call = False                   # (PPO's minibatch loop: not A2C's)
        prm, lr = self.policy.parameters(), cfg.learning_rate
        if cfg.optimizer == "rmsprop":
            self.opt = torch.optim.RMSprop(prm, lr=lr, alpha=cfg.rms_alpha, eps=cfg.rms_eps)
        elif cfg.optimizer == "rmsprop_tf":
            self.opt = RMSpropTFLike(prm, lr=lr, alpha=cfg.rms_alpha, eps=cfg.rms_eps)
        else:
            self.opt = torch.optim.Adam(prm, lr=lr, eps=1e-5)
        self.upd_stats = torch.zeros(8, dtype=torch.float32, device=env.device)
        self._it_graph, self._it_graph_key = None, None
        if self.fused_update and cfg.optimizer != "adam":     # RMSprop's one state vector in place of Adam's two
            del self.upd_m, self.upd_v
            self.upd_sq = torch.full((self.n_params,), 1.0 if cfg.optimizer == "rmsprop_tf" else 0.0,
                                     dtype=torch.float32, device=env.device)

    # ---------------------------------------------------------------- update --
    def _update_torch(self, N: int, T: int):
        """SB3 A2C.train on the first N rows of the rollout: one step of self.opt; the statistics into upd_stats"""
        c = self.cfg
        obs, act = self.obs_buf[:T].reshape(N, -1), self.act_buf[:T].reshape(N, -1)
        adv, ret = self.adv_buf[:T].reshape(N), self.ret_buf[:T].reshape(N)
        mean, value = self.policy(obs)
        logp = self.policy.log_prob(mean, act)
        a = (adv - adv.mean()) / (adv.std() + 1e-8) if c.normalize_advantage else adv
        pl = -(a * logp).mean()
        vf = ((ret - value) ** 2).mean()
        ent_loss = -self.policy.entropy()
        loss = pl + c.ent_coef * ent_loss + c.vf_coef * vf
        with torch.no_grad():
            zero = torch.zeros_like(pl)
            self.upd_stats.copy_(torch.stack([pl, vf, ent_loss, zero, zero, (a * logp).abs().mean(), zero, loss]))
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        if self.data_parallel:
            allreduce_gradients(self.policy.parameters(), self.group)
        nn.utils.clip_grad_norm_(self.policy.parameters(), c.max_grad_norm)
        self.opt.step()

    def _update_fused(self, N: int):
        """_update_torch as stream-ordered calls on self.flat[:n_params] (no host synchronisation): one
        b747_a2c_update; data-parallel, b747_a2c_grad, the all-reduce of the flat gradient and the optimiser's call with
        its 1 / world.  idx is NULL: the first N rows of the time-major buffers, in order."""
        c, p, L = self.cfg, _p, self._L
        stream = torch.cuda.current_stream().cuda_stream
        opt = A2C_OPTIMIZERS.index(c.optimizer)
        adam = c.optimizer == "adam"
        rows = (p(self.flat), self.env.obs_dim, p(self.obs_buf), p(self.act_buf), p(self.adv_buf), p(self.ret_buf), None,
                N, int(c.normalize_advantage), c.ent_coef, c.vf_coef, p(self.upd_ws), p(self.upd_grad), p(self.upd_stats))
        if not (self.data_parallel and dist.is_available() and dist.is_initialized()):
            self._lib.check(L.b747_a2c_update(
                *rows, opt, p(self.upd_m if adam else self.upd_sq), p(self.upd_v) if adam else None, p(self.upd_t),
                c.max_grad_norm, c.learning_rate, c.rms_alpha, 1e-5 if adam else c.rms_eps, stream), "b747_a2c_update")
            return
        self._lib.check(L.b747_a2c_grad(*rows, stream), "b747_a2c_grad")
        world = _world(self.group)
        dist.all_reduce(self.upd_grad, op=dist.ReduceOp.SUM, group=self.group)
        if adam:
            self._lib.check(L.b747_ppo_adam(
                p(self.flat), p(self.upd_m), p(self.upd_v), p(self.upd_t), p(self.upd_grad), self.n_params, 1.0 / world,
                c.max_grad_norm, c.learning_rate, 0.9, 0.999, 1e-5, stream), "b747_ppo_adam")
        else:
            self._lib.check(L.b747_ppo_rmsprop(
                p(self.flat), p(self.upd_sq), p(self.upd_t), p(self.upd_grad), self.n_params, 1.0 / world,
                c.max_grad_norm, c.learning_rate, c.rms_alpha, c.rms_eps, int(c.optimizer == "rmsprop_tf"), stream),
                "b747_ppo_rmsprop")

    def _update(self, T: int):
        """train()'s device work: the step, then the modules and the packed buffer brought up to date -- stream-ordered,
        and with fused_update free of host reads and synchronisation (learn(use_graph=True) captures it)"""
        N = T * self.env.n
        if self.fused_update:
            self._update_fused(N)
            load_flat(self.policy, self.flat)     # the flat vector is the master copy: hand it to the modules,
            self._lib.check(self._L.b747_policy_pack(   # and derive the packed sections the rollout kernels read
                self.flat.data_ptr(), self.env.obs_dim, torch.cuda.current_stream().cuda_stream), "b747_policy_pack")
        else:
            self._update_torch(N, T)
            self.sync_params()

    @torch.no_grad()
    def _train_stats(self, T: int) -> dict:
        """train()'s return value from upd_stats and the rollout buffers (one host synchronisation)"""
        N = T * self.env.n
        v, r = self.val_buf[:T].reshape(N), self.ret_buf[:T].reshape(N)
        var_r = r.var(unbiased=False)
        ev = 1 - (r - v).var(unbiased=False) / var_r if float(var_r) != 0 else torch.tensor(float("nan"))
        st = self.upd_stats.tolist()
        return {"policy_loss": st[0], "value_loss": st[1], "entropy_loss": st[2], "loss": st[7],
                "explained_variance": float(ev), "std": float(self.policy.log_std.exp().mean()), "pg_term_scale": st[5]}

    def train(self, T: Optional[int] = None):
        """One gradient step over all T * n rows of the rollout (SB3 1.4 A2C.train).  Returns SB3's train/* log values
        for A2C -- policy_loss, value_loss, entropy_loss, explained_variance (of the rollout's values against its
        returns), std and loss -- and, not an SB3 value, pg_term_scale = mean |A logp|, the magnitude of the terms the
        cancelling policy-loss mean sums (its float32 rounding scale)."""
        T = T or self.cfg.n_steps
        self._update(T)
        return self._train_stats(T)

    # ----------------------------------------------------------------- learn --
    def _iteration(self, T: int):
        """One iteration's device work: rollout, bootstrap value and GAE, update, repack"""
        self.collect_rollouts(T, use_graph=False)
        self.compute_gae(T)
        self._update(T)

    def _replay_iteration(self, T: int):
        """_iteration as one replay of a HIP graph captured on one stream (a linear graph: every call is stream-ordered
        behind the one before), captured when there is none for this key (PPO._graph_key; the capture launches nothing:
        the first iteration is a replay too).  The kernels read step_base, the parameters and the optimiser state on the
        device when they run."""
        key = self._graph_key(T)
        if self._it_graph is None or self._it_graph_key != key:
            s = torch.cuda.Stream(device=self.env.device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s), torch.no_grad():     # warm up the bootstrap forward's kernels (no state changes)
                self.policy(self.last_obs)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s), torch.no_grad():
                self._iteration(T)
            self._it_graph, self._it_graph_key = g, key
        self._it_graph.replay()

    def learn(self, iterations: int, n_steps: Optional[int] = None, control_test=None, use_graph: bool = False):
        """PPO.learn for A2C: `iterations` x (collect_rollouts, compute_gae, train) after an env reset; train()'s values
        per iteration, with mean_reward; control_test as PPO.learn's.  use_graph=True (needs fused_update=True and a
        rollout kernel: nothing of the iteration may run on the host) replays each iteration's device work as one HIP
        graph (_replay_iteration) and reads the statistics outside it; the same bits as use_graph=False.  The step
        tests stay outside the capture, before the iteration's replay.  With five-step rollouts an iteration is a
        handful of launches: this is the form A2C is meant to run in."""
        T = n_steps or self.cfg.n_steps
        assert T <= self.cfg.n_steps
        control_test = self.control_test if control_test is None else control_test
        pushes = _control_test_plan(self, control_test, iterations, T)
        if use_graph and not (self.fused_update and self.rollout_kernel):
            raise ValueError("A2C.learn(use_graph=True) needs fused_update=True and a rollout kernel (the torch update "
                             "and the two-launch rollout do host work that a capture would freeze)")
        self.last_obs.copy_(self.env.reset())
        self._last_obs_from_env = False
        hist = []
        for it in range(iterations):
            if pushes is not None and pushes[it]:
                control_test.evaluate(pushes[it])
            if use_graph:
                self._replay_iteration(T)
            else:
                self._iteration(T)
            hist.append(self._train_stats(T) | {"mean_reward": float(self.rew_buf[:T].mean())})
            if pushes is not None:
                hist[-1].update(control_test.history_entry())
        return hist


class PopulationPPO:
    """P independent PPO learners on ONE BatchControllerEnv, their rollouts flown side by side in one launch
    (b747_ppo_rollout_population, include/b747.h).

    Member p owns envs [p * envs_per_member, (p + 1) * envs_per_member) of `env`, its own policy (ActorCritic(obs_dim)
    built after torch.manual_seed(seeds[p]): what PPO(seed=seeds[p]) builds), its own reward constants
    (rew_configs[p], a reward_config dict as BatchControllerEnv.set_rew_config takes; None = the env's) and its own
    learning rate; gamma, gae_lambda, the clip range, the epochs and the batch size (rows of ONE member per minibatch) are
    cfg's, shared (the first three and the loss coefficients per member with `hyper`, below).  This is the shape of the reference's ControllerAgent.optimize() (neural/agent.py:89-136): trials
    that differ in reward_config and hyper-parameters, ranked by ControlTestCallback.mean_quality -- step_tests()
    here; ControlTest (below) keeps that callback's windows, its best quality and its saved model on the device.  The update is PPO(fused_update=True, epoch_call=True)'s, per member, from one C call per epoch
    (b747_ppo_epoch_population): the same kernels, the same bits as P separate learners
    (tests/test_gpu_ppo_population_train.py).  `seed` keys the action noise (Philox counters (seed, step, global env
    id), shared by the members, whose env ids differ).  No torch modules are kept: `flat` [P, stride] is the master copy
    of every member's parameters (member(p) gives an ActorCritic copy).

    batched_update=True (opt-in) makes the epoch call b747_ppo_epoch_batched: four launches per minibatch
    for all members (the member on blockIdx.y of member-batched update kernels) in place of four per member -- the same
    bits (tests/test_gpu_ppo_population_batched_train.py), a workspace slice per member instead of one shared.

    hyper (a list of one dict per member, as hyper_table takes) gives every member its own gamma,
    gae_lambda, clip_range, ent_coef, vf_coef, max_grad_norm and learning_rate -- the reference's PPO trial space
    (neural/setups.py, trial_hyperparams).  The values live in a [P, 8] float64 table, `hyper` on the CPU and
    `hyper_dev` on the env's device: compute_gae then is one b747_ppo_gae_population launch and the epoch call
    b747_ppo_epoch_population_hyper (b747_ppo_epoch_batched_hyper with batched_update) -- per member the bits of a
    separate learner with those values (tests/test_gpu_ppo_population_hyper_train.py).  set_hyper changes a member's
    values between iterations and copy_member copies one member onto another (the exploit step of a population-based
    schedule), neither rebuilding a buffer.  n_steps, batch_size, n_epochs and the network stay shared: they change
    shapes, not values.  With hyper=None nothing changes: the calls and the bits are those described above.

    sample_order="device" (opt-in) draws every epoch's sample orders for all members with ONE
    b747_ppo_sample_orders launch into the persistent `perm` buffer, in place of a torch.randperm per member, a stack and
    a gather on the host: a counter-based stream keyed by (seed, step_base, epoch, member), so the random streams are
    not the default's ("host": torch's generator, today's calls and bits) and train() takes no minibatch_order hook.  A
    member's rows are limited to 16,384 (n_steps * envs_per_member; the kernel sorts them in LDS).  With it no host
    randomness is left in an iteration, and learn(use_graph=True) replays rollout, GAE, the epochs and the repack as one
    HIP graph per iteration (with batched_update=True, whose calls read every per-member value on the device).

    exploit() is the exploit-and-explore step of a population-based schedule done on the device by one
    b747_ppo_exploit call -- the worst members by a device score re-seeded from the best, with perturbed table rows, no
    host read -- and `pop.pbt = PBT(interval)` makes learn() take that step every `interval` iterations."""

    # The batched update's workspace holds one slice per member (b747_ppo_epoch_batched_workspace: ~9 MB at the full
    # 256-workgroup grid, ~80 kB at batch 256) so that all members run in one launch; past this many bytes the call
    # works through the members in chunks of as many slices as fit, which changes no bit and costs four launches
    # per chunk and minibatch instead of four per minibatch.
    BATCHED_WORKSPACE_CAP = 1 << 30

    def __init__(self, env: BatchControllerEnv, n_members: int, envs_per_member: int = 64,
                 cfg: Optional[PPOConfig] = None, seeds=None, rew_configs=None, learning_rates=None, seed: int = 0,
                 batched_update: bool = False, hyper=None, sample_order: str = "host"):
        from . import _lib
        from .evaluate import pack_policies
        self._lib, self._L = _lib, _lib.lib()
        self.env, self.cfg, self.seed = env, cfg or PPOConfig(), int(seed)
        P, epp, n, od, dev = int(n_members), int(envs_per_member), env.n, env.obs_dim, env.device
        self.n_members, self.envs_per_member = P, epp
        if P < 1 or epp < 64 or epp % 64 != 0 or not ((P - 1) * epp < n <= P * epp):
            raise ValueError(f"PopulationPPO: {P} members of {epp} envs (a positive multiple of 64) do not tile the "
                             f"env's {n} envs (the last member may be partial)")
        if sample_order not in ("host", "device"):
            raise ValueError(f"PopulationPPO: sample_order={sample_order!r}: \"host\" or \"device\"")
        self.sample_order = sample_order
        self._graph, self._graph_key = None, None
        self.control_test = None          # a ControlTest that learn() flies and books before every iteration
        self.pbt = None                   # a PBT whose exploit steps learn() makes between iterations
        self._exploits, self._hyper_stale = 0, False
        if sample_order == "device":
            # the persistent order buffer, and the first draw into it (epoch 0 at step_base 0; train() draws again): the
            # entry point refuses a member of more rows than it sorts, or envs that the members do not cover, before
            # anything reaches the device
            self.perm = torch.empty(P, self.cfg.n_steps * epp, dtype=torch.int64, device=dev)
            if self._sample_orders(0, self.cfg.n_steps, None) != 0:
                raise ValueError(f"PopulationPPO(sample_order=\"device\"): {self._L.b747_last_error().decode()}")
        self.seeds = [self.seed + p for p in range(P)] if seeds is None else [int(s) for s in seeds]
        lrs = [self.cfg.learning_rate] * P if learning_rates is None else [float(x) for x in learning_rates]
        if len(self.seeds) != P or len(lrs) != P or (rew_configs is not None and len(rew_configs) != P):
            raise ValueError("PopulationPPO: seeds, rew_configs and learning_rates take one entry per member")
        # (hyper: the table holds every member's values; built first, so that a refused value raises before any launch)
        self.hyper = None if hyper is None else hyper_table(self.cfg, P, hyper, learning_rates)
        if self.hyper is not None:
            lrs = self.hyper[:, HYPER_COLUMN["learning_rate"]].tolist()
        self.learning_rates = lrs
        self._lr = (ctypes.c_double * P)(*lrs)            # b747_ppo_epoch_population reads them on the host
        nets = []
        for s in self.seeds:
            torch.manual_seed(s)
            nets.append(ActorCritic(od))
        self.n_params = sum(p.numel() for p in nets[0].flat_param_list())
        self.flat = pack_policies(nets, od, dev)          # [P, stride], one b747_policy_pack_batch launch
        self.stride = int(self.flat.shape[1])
        rows = [env.rew_constants(None if rew_configs is None else rew_configs[p]) for p in range(P)]
        self.rew = torch.tensor(rows, dtype=torch.float64, device=dev)
        self._rew_arg = None if rew_configs is None else self.rew     # (None: the kernel without the per-group loads)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        T = self.cfg.n_steps
        self.upd_m, self.upd_v, self.upd_grad = z(P, self.n_params), z(P, self.n_params), z(self.n_params)
        self.upd_t = torch.zeros(P, dtype=torch.int64, device=dev)
        ws = int(self._L.b747_ppo_update_workspace(od))
        if ws <= 0:
            raise ValueError(f"PopulationPPO does not cover this policy: {self._L.b747_last_error().decode()}")
        self.upd_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        self.batched_update = bool(batched_update)
        if self.batched_update:
            per = int(self._L.b747_ppo_epoch_batched_workspace(od, self.cfg.batch_size))
            if per <= 0:
                raise ValueError(f"PopulationPPO(batched_update=True): {self._L.b747_last_error().decode()}")
            self.lr_dev = torch.tensor(lrs, dtype=torch.float64, device=dev)      # b747_ppo_epoch_batched reads them there
            self.upd_ws_batched = torch.empty(max(1, min(P, self.BATCHED_WORKSPACE_CAP // per)) * per, dtype=torch.uint8,
                                              device=dev)
        self.hyper_dev = None if self.hyper is None else self.hyper.to(dev)   # the kernels read it there, when they run
        (self.obs_buf, self.act_buf, self.logp_buf, self.val_buf, self.rew_buf, self.done_buf, self.adv_buf,
         self.ret_buf) = _rollout_buffers(T, n, od, dev)
        self.last_val = z(n)
        if sample_order == "device":      # (persistent: a captured iteration writes it, the reductions read it afterwards)
            self.stats = z(self.cfg.n_epochs * P * -(-T * epp // self.cfg.batch_size) * 8)
        self.step_base = torch.zeros(1, dtype=torch.int64, device=dev)
        self.src_of = torch.arange(P, dtype=torch.int32, device=dev)      # exploit()'s result, persistent
        self.act_lo, self.act_hi = float(env.action_space.low), float(env.action_space.high)
        if self._rollout(0) != 0:                        # T = 0: validates the configuration, launches nothing
            raise ValueError(f"b747_ppo_rollout_population does not cover this env: {self._L.b747_last_error().decode()}")

    def _rollout(self, T: int) -> int:
        return self.env.ppo_rollout_population(
            T, self.flat, self.obs_buf, self.act_buf, self.logp_buf, self.val_buf, self.rew_buf, self.done_buf,
            seed=self.seed, step_base=self.step_base, envs_per_policy=self.envs_per_member, rew_pop=self._rew_arg,
            last_val=self.last_val, act_lo=self.act_lo, act_hi=self.act_hi, check=False)

    @torch.no_grad()
    def collect_rollouts(self, n_steps: Optional[int] = None):
        """n_steps (default cfg.n_steps) policy + env steps of every member: one b747_ppo_rollout_population call.  It
        also leaves the bootstrap values in last_val and advances step_base."""
        T = n_steps or self.cfg.n_steps
        assert T <= self.cfg.n_steps
        self._lib.check(self._rollout(T), "b747_ppo_rollout_population")
        return T

    @torch.no_grad()
    def compute_gae(self, T: Optional[int] = None):
        """PPO.compute_gae for every member: one b747_ppo_gae launch over all N envs, bootstrapped with the rollout
        kernel's last_val (with hyper: one b747_ppo_gae_population launch, each member's gamma and gae_lambda from its
        row of hyper_dev)"""
        T, c, p = T or self.cfg.n_steps, self.cfg, _p
        if self.hyper is not None:
            self._lib.check(self._L.b747_ppo_gae_population(
                p(self.rew_buf), p(self.val_buf), p(self.done_buf), p(self.last_val), T, self.env.n, self.n_members,
                self.envs_per_member, p(self.hyper_dev), p(self.adv_buf), p(self.ret_buf),
                torch.cuda.current_stream().cuda_stream), "b747_ppo_gae_population")
            return
        self._lib.check(self._L.b747_ppo_gae(
            p(self.rew_buf), p(self.val_buf), p(self.done_buf), p(self.last_val), T, self.env.n, c.gamma, c.gae_lambda,
            p(self.adv_buf), p(self.ret_buf), torch.cuda.current_stream().cuda_stream), "b747_ppo_gae")

    def member_rows(self, T: int) -> torch.Tensor:
        """[P, T * envs_per_member] the rollout rows t * N + p * envs_per_member + j of each member, in the order
        (t, j) of a learner that had the member's envs to itself"""
        P, epp, dev = self.n_members, self.envs_per_member, self.env.device
        t = torch.arange(T, device=dev)[None, :, None] * self.env.n
        return (t + torch.arange(P, device=dev)[:, None, None] * epp + torch.arange(epp, device=dev)[None, None]) \
            .reshape(P, T * epp)

    @torch.no_grad()
    def train(self, T: Optional[int] = None,
              minibatch_order: Optional[Callable[[int, int, int, int], torch.Tensor]] = None):
        """PPO.train(fused_update, epoch_call) for every member: per epoch one sample order per member and ONE
        b747_ppo_epoch_population call (b747_ppo_epoch_batched with batched_update; their _hyper forms with hyper, which
        take the members' values from the table); afterwards one b747_policy_pack_batch.
        minibatch_order(epoch, T, envs_per_member, p) -> [T * envs_per_member] indices into MEMBER p's own time-major
        rows (t * envs_per_member + j: what PPO.train's hook gives a learner that has the member's envs to itself);
        default torch.randperm.  With sample_order="device" the orders are one b747_ppo_sample_orders launch per epoch
        (seed, step_base and the epoch key them; no hook).  Returns PPO.train's names as [P] tensors (float64;
        explained_variance and std float32-derived), per member."""
        T = T or self.cfg.n_steps
        return self._train_stats(T, self._epochs(T, minibatch_order))

    def _sample_orders(self, epoch: int, T: int, step_base: Optional[torch.Tensor]) -> int:
        """One b747_ppo_sample_orders call into perm: every member's order of its T * envs_per_member rows for `epoch`;
        the library's return code"""
        dev = self.perm.device
        return int(self._L.b747_ppo_sample_orders(
            _p(self.perm), self.n_members, T, self.envs_per_member, self.env.n, self.seed & 0xFFFFFFFFFFFFFFFF,
            None if step_base is None else _p(step_base), epoch,
            torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None))

    @torch.no_grad()
    def _epochs(self, T: int, minibatch_order=None) -> torch.Tensor:
        """train()'s device work: per epoch the sample orders and the epoch call, then the repack -- stream-ordered, and
        with sample_order="device" free of host randomness, allocations and synchronisation (learn(use_graph=True)
        captures it).  Returns the statistics [n_epochs, P, n_mb, 8] (with "device": a view of the persistent buffer)."""
        c, P, epp = self.cfg, self.n_members, self.envs_per_member
        if self.env.n != P * epp:
            raise ValueError("PopulationPPO.train: every member needs envs_per_member envs (one n_rows for all members)")
        device_order = self.sample_order == "device"
        if device_order and minibatch_order is not None:
            raise ValueError("PopulationPPO.train: minibatch_order with sample_order=\"device\" (the orders are "
                             "b747_ppo_sample_orders'; build the population with sample_order=\"host\" to pass a hook)")
        dev, n_rows, p = self.env.device, T * epp, _p
        n_mb = -(-n_rows // c.batch_size)
        if device_order:
            assert T <= c.n_steps
            stats = self.stats[:c.n_epochs * P * n_mb * 8].view(c.n_epochs, P, n_mb, 8)
        else:
            rows_of = self.member_rows(T)
            stats = torch.empty(c.n_epochs, P, n_mb, 8, dtype=torch.float32, device=dev)
        for epoch in range(c.n_epochs):
            if device_order:
                self._lib.check(self._sample_orders(epoch, T, self.step_base), "b747_ppo_sample_orders")
                perm = self.perm          # (its first P * n_rows entries: [P][n_rows], rows t * N + i of the buffers)
            else:
                if minibatch_order is None:
                    local = torch.stack([torch.randperm(n_rows, device=dev) for _ in range(P)])
                else:
                    local = torch.stack([torch.as_tensor(minibatch_order(epoch, T, epp, m), device=dev).to(torch.int64)
                                         for m in range(P)])
                assert tuple(local.shape) == (P, n_rows), "minibatch_order must give every row of the member once"
                perm = torch.gather(rows_of, 1, local).contiguous()   # member rows -> rows t * N + i of the buffers
            if self.hyper is not None:
                head = (p(self.flat), P, self.stride, self.env.obs_dim, p(self.obs_buf), p(self.act_buf),
                        p(self.logp_buf), p(self.adv_buf), p(self.ret_buf), p(perm), n_rows, c.batch_size)
                tail = (p(self.upd_m), p(self.upd_v), p(self.upd_t), 0.9, 0.999, 1e-5, p(stats[epoch]),
                        torch.cuda.current_stream().cuda_stream)
                if self.batched_update:
                    self._lib.check(self._L.b747_ppo_epoch_batched_hyper(
                        *head, p(self.hyper_dev), p(self.upd_ws_batched), self.upd_ws_batched.numel(), *tail),
                        "b747_ppo_epoch_batched_hyper")
                else:       # (the host table: this call reads it before it returns)
                    self._lib.check(self._L.b747_ppo_epoch_population_hyper(
                        *head, p(self.hyper), p(self.upd_ws), p(self.upd_grad), *tail), "b747_ppo_epoch_population_hyper")
                continue
            if self.batched_update:
                self._lib.check(self._L.b747_ppo_epoch_batched(
                    p(self.flat), P, self.stride, self.env.obs_dim, p(self.obs_buf), p(self.act_buf), p(self.logp_buf),
                    p(self.adv_buf), p(self.ret_buf), p(perm), n_rows, c.batch_size, c.clip_range, c.ent_coef, c.vf_coef,
                    p(self.upd_ws_batched), self.upd_ws_batched.numel(), p(self.upd_m), p(self.upd_v), p(self.upd_t),
                    c.max_grad_norm, p(self.lr_dev), 0.9, 0.999, 1e-5, p(stats[epoch]),
                    torch.cuda.current_stream().cuda_stream), "b747_ppo_epoch_batched")
                continue
            self._lib.check(self._L.b747_ppo_epoch_population(
                p(self.flat), P, self.stride, self.env.obs_dim, p(self.obs_buf), p(self.act_buf), p(self.logp_buf),
                p(self.adv_buf), p(self.ret_buf), p(perm), n_rows, c.batch_size, c.clip_range, c.ent_coef, c.vf_coef,
                p(self.upd_ws), p(self.upd_grad), p(self.upd_m), p(self.upd_v), p(self.upd_t), c.max_grad_norm, self._lr,
                0.9, 0.999, 1e-5, p(stats[epoch]), torch.cuda.current_stream().cuda_stream), "b747_ppo_epoch_population")
        self.repack()
        return stats

    @torch.no_grad()
    def _train_stats(self, T: int, stats: torch.Tensor) -> dict:
        """train()'s return value from the epochs' statistics [n_epochs, P, n_mb, 8] and the rollout buffers"""
        P, epp = self.n_members, self.envs_per_member
        st = stats.double()
        mean, last = st.mean(dim=(0, 2)), st[-1].mean(dim=1)          # [P, 8]: every minibatch / the last epoch's
        v = self.val_buf[:T].reshape(T, P, epp).permute(1, 0, 2).reshape(P, -1)
        r = self.ret_buf[:T].reshape(T, P, epp).permute(1, 0, 2).reshape(P, -1)
        var_r = r.var(dim=1, unbiased=False)
        ev = torch.where(var_r != 0, 1 - (r - v).var(dim=1, unbiased=False) / var_r, torch.full_like(var_r, float("nan")))
        return _train_log(mean.unbind(1), (last[:, 4], last[:, 6]), st[-1, :, -1, 7], ev,
                          self.flat[:, self.n_params - 1].exp())

    def repack(self):
        """Derive the packed sections of every member from its flat parameters (after an update): one launch"""
        self._lib.check(self._L.b747_policy_pack_batch(self.flat.data_ptr(), self.env.obs_dim, self.n_members, self.stride,
                                                       torch.cuda.current_stream().cuda_stream), "b747_policy_pack_batch")

    def _iteration_graph_key(self, T: int):
        """What a captured iteration baked in (PPO._graph_key): the step count, the env's C descriptor, configuration
        and constants, and the kernel specialisation"""
        env = self.env
        return (T, env._batch(), bytes(env.cfg), bytes(env.consts), int(self._L.b747_get_specialization()))

    def _replay_iteration(self, T: int) -> torch.Tensor:
        """One iteration's device work -- rollout, GAE, n_epochs x (orders + epoch call), repack -- as one replay of a
        HIP graph captured on one stream (a linear graph: every call is stream-ordered behind the one before), captured
        when there is none for this key (the capture launches nothing; the first iteration is a replay too).  The
        kernels read step_base, the hyper-parameter table, the learning rates, the parameters and the Adam state on the
        device when they run: set_hyper and copy_member between replays are stream-ordered copies into buffers the
        graph already addresses.  Returns the statistics (_epochs': a view of the persistent buffer)."""
        key = self._iteration_graph_key(T)
        if self._graph is None or self._graph_key != key:
            s = torch.cuda.Stream(device=self.env.device)
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s), torch.no_grad():
                self.collect_rollouts(T)
                self.compute_gae(T)
                stats = self._epochs(T)
            self._graph, self._graph_key, self._graph_stats = g, key, stats
        self._graph.replay()
        return self._graph_stats

    def learn(self, iterations: int, n_steps: Optional[int] = None, minibatch_order=None, use_graph: bool = False):
        """`iterations` x (collect_rollouts, compute_gae, train) after an env reset; train()'s values per iteration, with
        mean_reward.  use_graph=True (needs sample_order="device" and batched_update=True: the other epoch calls take
        the learning rates or the table from the host, which a capture would freeze) replays each iteration's device
        work as one HIP graph (_replay_iteration) and computes the statistics outside it, from the persistent
        buffers; the same bits as use_graph=False.
        self.control_test (a ControlTest built for this population, attached as `pop.control_test = ControlTest(pop,
        ...)`; None, the default = today's calls, bits and keys; an attribute, not a keyword as PPO.learn
        has it: this method's parameter list is pinned by tests/test_ppo_sample_orders_abi.py):
        before an iteration's device work -- outside the captured iteration, before its replay -- it flies the step
        tests with the policies the rollout is about to use and books them as often as the reference's callback would
        evaluate during that rollout (control_test_pushes; none launches nothing, more than 256 is a ValueError here).
        The iteration's entry gains transfer_settling_time / transfer_overshoot / transfer_quality: [P] device clones of
        the windowed means after those pushes, NaN until the first evaluation."""
        T, P, epp = n_steps or self.cfg.n_steps, self.n_members, self.envs_per_member
        control_test = self.control_test
        pushes = _control_test_plan(self, control_test, iterations, T)
        if use_graph:
            if self.sample_order != "device":
                raise ValueError("PopulationPPO.learn(use_graph=True) needs sample_order=\"device\" (the host's "
                                 "torch.randperm draws cannot be captured)")
            if not self.batched_update:
                raise ValueError("PopulationPPO.learn(use_graph=True) needs batched_update=True (the other epoch calls "
                                 "read the learning rates or the hyper-parameter table on the host: a capture would "
                                 "freeze them)")
        if minibatch_order is not None and self.sample_order == "device":
            raise ValueError("PopulationPPO.learn: minibatch_order with sample_order=\"device\" (the orders are "
                             "b747_ppo_sample_orders')")
        assert T <= self.cfg.n_steps
        self._pbt_check()
        self.env.reset()
        hist = []
        for it in range(iterations):
            if pushes is not None and pushes[it]:
                control_test.evaluate(pushes[it])
            source = self._pbt_step(it, hist)
            if use_graph:
                st = self._train_stats(T, self._replay_iteration(T))
            else:
                self.collect_rollouts(T)
                self.compute_gae(T)
                st = self.train(T, minibatch_order)
            st["mean_reward"] = self.rew_buf[:T].reshape(T, P, epp).mean(dim=(0, 2))
            if pushes is not None:
                st.update(control_test.history_entry())
            if source is not None:
                st["pbt_source"] = source
            hist.append(st)
        return hist

    # ------------------------------------------------------------------ exploit and explore --
    _HYPER_KEYS = HYPER_COLUMN
    _check_value = staticmethod(_check_hyper_value)
    PBT_EXPLORE = PBT_EXPLORE

    def _table_on_device(self) -> bool:
        """Whether the update reads the hyper-parameter table on the device (the batched epoch call does; the other one
        reads the HOST table, which a device step cannot update)"""
        return bool(self.batched_update)

    def _state_rows(self):
        """The two optimiser state buffers [P, n_params] that travel with a member (Adam's m and v)"""
        return self.upd_m, self.upd_v

    def _exploit_args(self, fraction, explore, rewards):
        """exploit()'s host-side checks, all before any device work: (n_replace, the explore rows or None)"""
        name, P = type(self).__name__, self.n_members
        if self.hyper is not None and not self._table_on_device():
            raise ValueError(f"{name}.exploit needs batched_update=True (the other epoch call reads the "
                             "hyper-parameter table on the host, which a step on the device cannot update)")
        n_replace = int(P * float(fraction))
        if not 1 <= n_replace <= P // 2:
            raise ValueError(f"{name}.exploit: fraction={fraction} replaces {n_replace} of {P} members (at least 1, at "
                             f"most {P // 2}: winners and losers must be disjoint)")
        if self.hyper is None:
            if explore is not None:
                raise ValueError(f"{name}.exploit: explore on a population built with hyper=None (it has no table: it "
                                 "exploits parameters and optimiser state only)")
            rows = None
        else:
            rule = self.PBT_EXPLORE if explore is None else dict(explore)
            rows = explore_table(self._HYPER_KEYS, self._check_value, rule, f"{name}.exploit") if rule else None
        if rewards and self._rew_arg is None:
            raise ValueError(f"{name}.exploit: rewards=True on a population built without rew_configs (its rollout "
                             "kernel reads no per-member reward constants)")
        return n_replace, rows

    @torch.no_grad()
    def exploit(self, score=None, fraction: float = 0.25, explore=None, rewards: bool = False, round=None):
        """The exploit-and-explore step of a truncation-selection population-based schedule (Jaderberg et al., 2017),
        decided and done on the device by one b747_ppo_exploit call (include/b747.h states the contract):
        the n_replace = int(P * fraction) worst members by `score` are each re-seeded from one of the n_replace best,
        drawn at random (a counter-based stream keyed by seed, step_base, `round` and the member), if that one is
        strictly better.  A replaced member takes its source's parameters (the whole stride of flat), optimiser state
        rows, step count and table row, the row's columns perturbed by `explore`.  No host read, no synchronisation.

        score: a [P] float64 device tensor, higher is better, NaN ranks last; default self.control_test.objective(),
        the windowed transfer quality (ValueError without a control test or before its first evaluation -- the host's
        count of them).  explore: a dict key -> (f_lo, f_hi, min, max) over the class's hyper keys: the copied value
        times f_lo or f_hi (a fair coin per column), clamped to [min, max]; keys not named are copied unchanged, {}
        copies every column; default PBT_EXPLORE (learning_rate and ent_coef at 0.8 / 1.2 -- the paper's convention,
        not a measured choice -- inside the reference's trial ranges).  A population built with hyper=None takes no
        explore.  rewards=True also moves the source's reward constants (`rew`; needs rew_configs); by default a
        member's reward constants are its own.  round: default the number of exploit calls so far.
        With a table PopulationPPO needs batched_update=True.  An attached control test's window books (ring, count,
        last, window_mean) follow the policy; best_quality, best_eval and best_flat stay the slot's own.  Afterwards
        the CPU mirrors (hyper, learning_rates) are stale until sync_hyper().
        Returns src_of, [P] int32, a persistent device buffer: src_of[p] = the member p was replaced from, or p."""
        n_replace, rows = self._exploit_args(fraction, explore, rewards)
        name, P, p = type(self).__name__, self.n_members, _p
        ct = self.control_test
        if score is None:
            if ct is None:
                raise ValueError(f"{name}.exploit: no score and no control test (attach one, or pass score=)")
            if ct.evaluations == 0:
                raise ValueError(f"{name}.exploit: the control test has not evaluated yet (its objective is NaN)")
            score = ct.objective()
        if not (isinstance(score, torch.Tensor) and score.dtype == torch.float64 and tuple(score.shape) == (P,)
                and score.device == self.flat.device):
            raise ValueError(f"{name}.exploit: score is a [{P}] float64 tensor on {self.flat.device}")
        score = score.contiguous()
        arr = None if rows is None else (ctypes.c_double * (4 * HYPER_COLS))(*[x for row in rows for x in row])
        s0, s1 = self._state_rows()
        self._lib.check(self._L.b747_ppo_exploit(
            p(score), P, n_replace, self.seed & 0xFFFFFFFFFFFFFFFF, p(self.step_base),
            (self._exploits if round is None else int(round)) & 0xFFFFFFFF, p(self.flat), self.stride, p(s0), p(s1),
            self.n_params, p(self.upd_t), None if self.hyper is None else p(self.hyper_dev), arr,
            p(self.rew) if rewards else None, p(self.src_of), torch.cuda.current_stream().cuda_stream),
            "b747_ppo_exploit")
        self._exploits += 1
        self._hyper_stale = self.hyper is not None
        if ct is not None:          # (small: torch gathers on the stream)
            idx = self.src_of.long()
            ct.ring.copy_(ct.ring[:, idx])
            for x in (ct.count, ct.last, ct.window_mean):
                x.copy_(x[idx])
        return self.src_of

    def sync_hyper(self):
        """Bring the CPU mirrors (hyper, learning_rates) up to date with hyper_dev after a device exploit: one
        device-to-host copy -- a HOST READ, the only one of this feature; set_hyper, copy_member and
        PopulationA2C.optimizers make it when the mirror is stale, nothing else does."""
        if self.hyper is not None:
            self.hyper.copy_(self.hyper_dev)
            for p, lr in enumerate(self.hyper[:, 0].tolist()):        # (column 0: learning_rate, in both key sets)
                self.learning_rates[p] = lr
                self._lr[p] = lr
        self._hyper_stale = False

    def _pbt_check(self):
        """learn()'s checks of self.pbt before any device work"""
        pbt = getattr(self, "pbt", None)
        if pbt is None:
            return
        self._exploit_args(pbt.fraction, pbt.explore, pbt.rewards)
        if pbt.score == "transfer_quality" and self.control_test is None:
            raise ValueError(f"{type(self).__name__}.learn: pbt ranks by transfer_quality, which needs a control test "
                             "(attach one, or use PBT(score=\"mean_reward\"))")

    def _pbt_step(self, it: int, hist: list):
        """The exploit step learn() makes before iteration `it`'s device work where self.pbt asks for one and a score
        exists; the iteration's pbt_source entry (a [P] int32 device clone of src_of, arange(P) where no exploit ran),
        or None without a pbt"""
        pbt = getattr(self, "pbt", None)
        if pbt is None:
            return None
        if it > 0 and it % pbt.interval == 0:
            if pbt.score == "mean_reward":
                score = hist[-1]["mean_reward"].double()
            else:
                score = None if self.control_test.evaluations > 0 else False
            if score is not False:
                return self.exploit(score, pbt.fraction, pbt.explore, pbt.rewards).clone()
        return torch.arange(self.n_members, dtype=torch.int32, device=self.flat.device)

    def _need_hyper(self, what: str, *members):
        if self.hyper is None:
            raise ValueError(f"PopulationPPO.{what}: the population was built with hyper=None (its hyper-parameters are "
                             f"cfg's, kernel arguments shared by the members)")
        for m in members:
            if not 0 <= int(m) < self.n_members:
                raise ValueError(f"PopulationPPO.{what}: member {m} of {self.n_members}")

    def set_hyper(self, p: int, **kw):
        """Change hyper-parameters of member p (keys as hyper_table's, validated the same way): the CPU row, then one
        stream-ordered copy of that row into hyper_dev -- the launches that follow on the stream read the new values.
        No buffer is rebuilt, and a captured graph of the population's calls stays valid (the kernels read the table
        when they run)."""
        self._need_hyper("set_hyper", p)
        if getattr(self, "_hyper_stale", False):
            self.sync_hyper()
        unknown = sorted(set(kw) - set(HYPER_COLUMN))
        if unknown:
            raise ValueError(f"PopulationPPO.set_hyper: unknown key(s) {unknown}; a member's own values are "
                             f"{sorted(HYPER_COLUMN)}")
        new = {k: _check_hyper_value(k, x, f"PopulationPPO.set_hyper: member {p}") for k, x in kw.items()}
        for k, x in new.items():            # (nothing is written before every value has passed)
            self.hyper[p, HYPER_COLUMN[k]] = x
        self.learning_rates[p] = float(self.hyper[p, HYPER_COLUMN["learning_rate"]])
        self._lr[p] = self.learning_rates[p]
        self.hyper_dev[p].copy_(self.hyper[p], non_blocking=True)

    def copy_member(self, src: int, dst: int, hyper: bool = True):
        """Member src's parameters (the whole stride of flat: the packed sections travel with them), Adam moments and
        step count onto member dst, and with `hyper` its table row too: device copies on the current stream, no
        synchronisation -- the exploit step of a population-based schedule, and what optimize()'s "keep the best"
        needs.  The members' envs, reward constants and rollout rows stay their own."""
        self._need_hyper("copy_member", src, dst)
        if getattr(self, "_hyper_stale", False):
            self.sync_hyper()
        if int(src) == int(dst):
            return
        for x in (self.flat, self.upd_m, self.upd_v, self.upd_t):
            x[dst].copy_(x[src])
        if hyper:
            self.hyper[dst] = self.hyper[src]
            self.learning_rates[dst] = self.learning_rates[src]
            self._lr[dst] = self._lr[src]
            self.hyper_dev[dst].copy_(self.hyper_dev[src])

    def member(self, p: int) -> ActorCritic:
        """A copy of member p's policy as an ActorCritic on the env's device"""
        net = ActorCritic(self.env.obs_dim).to(self.env.device)
        load_flat(net, self.flat[p])
        return net

    def step_tests(self, vartheta_ref, state0=(0, 11000, 250, 0, 0, 0), tk: Optional[float] = None, **kwargs):
        """PPO.step_tests for every member in ONE launch (evaluate.population_step_tests on the packed buffer): the
        reference's ControlTestCallback metrics as [P, R], its means "mean_quality" / "mean_overshoot" /
        "mean_settling_time" as [P] and "best", the member optimize() would keep."""
        from .evaluate import population_step_tests
        e = self.env
        kw = _step_test_kwargs(e) | kwargs
        return population_step_tests(self.flat, vartheta_ref, state0=state0, tk=e.tk if tk is None else tk, **kw)


# The hyper-parameter table of a population of A2C learners: PPO's layout (HYPER_COLS, HYPER_COLUMN)
# without clip_range -- column 1 is 0 -- and with the member's optimiser, its B747_OPT_* value, in column 7
# (include/b747.h B747_PPO_HYPER_OPTIMIZER).  The keys are A2CConfig's names.
A2C_HYPER_COLUMN = {"learning_rate": 0, "ent_coef": 2, "vf_coef": 3, "max_grad_norm": 4, "gamma": 5, "gae_lambda": 6,
                    "optimizer": 7}


def _check_a2c_hyper_value(key: str, x, where: str) -> float:
    """x as the table's float if it is a value `key` may take: an A2C_OPTIMIZERS name for "optimizer" (stored as its
    index, the B747_OPT_* value), _check_hyper_value's ranges for the others"""
    if key != "optimizer":
        return _check_hyper_value(key, x, where)
    if x not in A2C_OPTIMIZERS:
        raise ValueError(f"{where}: optimizer = {x!r}: one of {list(A2C_OPTIMIZERS)}")
    return float(A2C_OPTIMIZERS.index(x))


def a2c_hyper_table(cfg: A2CConfig, n_members: int, hyper=None, learning_rates=None) -> torch.Tensor:
    """hyper_table for A2C learners: the [n_members, 8] float64 CPU table with columns A2C_HYPER_COLUMN (column 1, PPO's
    clip_range, is 0).  hyper: None (every row is cfg's) or one dict per member with keys among learning_rate,
    ent_coef, vf_coef, max_grad_norm, gamma, gae_lambda and optimizer (an A2C_OPTIMIZERS name); a key a member does not
    name comes from cfg -- the learning rate from learning_rates[p] where that list is given (then no dict may name
    learning_rate: one source per value).  ValueError for an unknown key (clip_range is one: A2C has none), a list of the
    wrong length, an unknown optimizer or a value outside its range.  n_steps, normalize_advantage, rms_alpha, rms_eps
    and the network are not keys: they stay the population's."""
    P = int(n_members)
    if P < 1:
        raise ValueError(f"a2c_hyper_table: {P} members")
    rows = [{}] * P if hyper is None else list(hyper)
    if len(rows) != P or (learning_rates is not None and len(learning_rates) != P):
        raise ValueError("a2c_hyper_table: hyper and learning_rates take one entry per member")
    table = torch.zeros(P, HYPER_COLS, dtype=torch.float64)
    for p, row in enumerate(rows):
        unknown = sorted(set(row) - set(A2C_HYPER_COLUMN))
        if unknown:
            raise ValueError(f"a2c_hyper_table: member {p}: unknown key(s) {unknown}; a member's own values are "
                             f"{sorted(A2C_HYPER_COLUMN)} (n_steps, normalize_advantage, RMSprop's alpha and eps and "
                             f"the network are shared; A2C has no clip_range)")
        if learning_rates is not None and "learning_rate" in row:
            raise ValueError(f"a2c_hyper_table: member {p} names learning_rate although learning_rates is given")
        for key, col in A2C_HYPER_COLUMN.items():
            if key in row:
                x = row[key]
            elif key == "learning_rate" and learning_rates is not None:
                x = learning_rates[p]
            else:
                x = getattr(cfg, key)
            table[p, col] = _check_a2c_hyper_value(key, x, f"a2c_hyper_table: member {p}")
    return table


class PopulationA2C(PopulationPPO):
    """P independent A2C learners on ONE BatchControllerEnv: PopulationPPO's members -- their envs,
    policies from `seeds`, reward constants from `rew_configs`, the one-launch rollout with its bootstrap values
    (b747_ppo_rollout_population), step_tests, member, repack -- with A2C's update: ONE gradient step per rollout over a
    member's n_steps * envs_per_member rows, for all members from one b747_a2c_update_population call (include/b747.h;
    the member on blockIdx.y of member-batched siblings of b747_a2c_update's kernels).  This is the shape of the
    reference's ControllerAgent.optimize() with its default net_class=A2C: trials that differ in reward_config and in
    gamma, gae_lambda, max_grad_norm, learning_rate, ent_coef, vf_coef and the optimiser (neural/setups.py,
    trial_hyperparams), ranked by a ControlTest (`pop.control_test = ControlTest(pop, ...)`, as for PopulationPPO).

    The population always has a hyper-parameter table (a2c_hyper_table: `hyper` [P, 8] on the CPU, `hyper_dev` on the
    env's device; hyper=None makes every row cfg's): the GAE is one b747_ppo_gae_population launch and the update reads
    each member's ent_coef, vf_coef, max_grad_norm, learning rate and optimiser from its row on the device.  Shared:
    n_steps, normalize_advantage, rms_alpha, rms_eps and the network; Adam is eps 1e-5 with betas 0.9 / 0.999, as in
    A2C.  The optimiser state is upd_s0 and upd_s1 [P, n_params] (RMSprop's square average -- ONES at first for an
    "rmsprop_tf" member -- or Adam's m in upd_s0, Adam's v in upd_s1) with the step counts upd_t [P]; `stats` [P, 8] is
    the persistent statistics buffer (b747_a2c_grad's row per member); `rows` [P, n_steps * envs_per_member] is the
    members' index table (member_rows), built once.  Per member the bits are those of a separate learner composed from
    the single-learner calls with the member's values (tests/test_gpu_a2c_population_train.py).

    train() draws no sample order (A2C takes the whole rollout, in order): there is no minibatch_order or sample_order
    here, and passing one is a ValueError.  learn(use_graph=True) replays rollout, GAE, update and repack as one HIP
    graph per iteration."""

    def __init__(self, env: BatchControllerEnv, n_members: int, envs_per_member: int = 64,
                 cfg: Optional[A2CConfig] = None, seeds=None, rew_configs=None, learning_rates=None, seed: int = 0,
                 hyper=None, **unsupported):
        self._refuse("PopulationA2C", unsupported)
        cfg = cfg or A2CConfig()
        if cfg.optimizer not in A2C_OPTIMIZERS:
            raise ValueError(f"A2CConfig.optimizer={cfg.optimizer!r}: \"rmsprop\", \"rmsprop_tf\" or \"adam\"")
        P = int(n_members)
        # (the table first, so that a refused value raises before any launch; a bad member count is the parent's to name)
        table = a2c_hyper_table(cfg, P, hyper, learning_rates) if P >= 1 else None
        super().__init__(env, P, envs_per_member, cfg, seeds=seeds, rew_configs=rew_configs,
                         learning_rates=learning_rates, seed=seed)
        dev, od, epp = env.device, env.obs_dim, self.envs_per_member
        if env.n != P * epp:
            raise ValueError(f"PopulationA2C: every member needs envs_per_member envs ({P} x {epp} != {env.n}: one "
                             "batch for all members)")
        del self.upd_m, self.upd_v            # (Adam's two of the parent: the state rows below take their place)
        self.hyper, self.hyper_dev = table, table.to(dev)
        self.learning_rates = table[:, A2C_HYPER_COLUMN["learning_rate"]].tolist()
        for p, lr in enumerate(self.learning_rates):
            self._lr[p] = lr
        tf = table[:, A2C_HYPER_COLUMN["optimizer"]] == A2C_OPTIMIZERS.index("rmsprop_tf")
        self.upd_s0 = tf.to(torch.float32)[:, None].expand(P, self.n_params).contiguous().to(dev)
        self.upd_s1 = torch.zeros(P, self.n_params, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(P, 8, dtype=torch.float32, device=dev)
        self.rows = self.member_rows(cfg.n_steps).contiguous()
        per = int(self._L.b747_ppo_epoch_batched_workspace(od, max(2, cfg.n_steps * epp)))
        if per <= 0:
            raise ValueError(f"PopulationA2C: {self._L.b747_last_error().decode()}")
        self.upd_ws_batched = torch.empty(max(1, min(P, self.BATCHED_WORKSPACE_CAP // per)) * per, dtype=torch.uint8,
                                          device=dev)

    @staticmethod
    def _refuse(what: str, kw: dict):
        """A2C draws no sample order and has one update path: the keywords PopulationPPO takes for those are refused"""
        if kw:
            raise ValueError(f"{what}: {sorted(kw)} not taken (A2C's one gradient step reads a member's whole rollout in "
                             "order: there is no minibatch_order, sample_order or batched_update here)")

    @property
    def optimizers(self) -> list:
        """Every member's optimiser by name (from the CPU table, brought up to date first after a device exploit:
        sync_hyper, a host read)"""
        if getattr(self, "_hyper_stale", False):
            self.sync_hyper()
        return [A2C_OPTIMIZERS[int(k)] for k in self.hyper[:, A2C_HYPER_COLUMN["optimizer"]].tolist()]

    @torch.no_grad()
    def _update(self, T: int):
        """train()'s device work: one b747_a2c_update_population call on the first T * envs_per_member entries of every
        member's row of `rows`, then the repack -- stream-ordered, no host read, allocation or synchronisation
        (learn(use_graph=True) captures it)"""
        c, p = self.cfg, _p
        assert T <= c.n_steps
        self._lib.check(self._L.b747_a2c_update_population(
            p(self.flat), self.n_members, self.stride, self.env.obs_dim, p(self.obs_buf), p(self.act_buf),
            p(self.adv_buf), p(self.ret_buf), p(self.rows), self.rows.shape[1], T * self.envs_per_member,
            int(c.normalize_advantage), p(self.hyper_dev), p(self.upd_ws_batched), self.upd_ws_batched.numel(),
            p(self.upd_s0), p(self.upd_s1), p(self.upd_t), c.rms_alpha, c.rms_eps, 0.9, 0.999, 1e-5, p(self.stats),
            torch.cuda.current_stream().cuda_stream), "b747_a2c_update_population")
        self.repack()

    @torch.no_grad()
    def _train_stats(self, T: int) -> dict:
        """train()'s return value from `stats` and the rollout buffers: A2C.train's names as [P] tensors"""
        P, epp = self.n_members, self.envs_per_member
        st = self.stats.double()
        v = self.val_buf[:T].reshape(T, P, epp).permute(1, 0, 2).reshape(P, -1)
        r = self.ret_buf[:T].reshape(T, P, epp).permute(1, 0, 2).reshape(P, -1)
        var_r = r.var(dim=1, unbiased=False)
        ev = torch.where(var_r != 0, 1 - (r - v).var(dim=1, unbiased=False) / var_r, torch.full_like(var_r, float("nan")))
        return {"policy_loss": st[:, 0], "value_loss": st[:, 1], "entropy_loss": st[:, 2], "loss": st[:, 7],
                "explained_variance": ev, "std": self.flat[:, self.n_params - 1].exp(), "pg_term_scale": st[:, 5]}

    def train(self, T: Optional[int] = None, **unsupported):
        """A2C.train for every member: ONE b747_a2c_update_population call, then one b747_policy_pack_batch.  Returns
        A2C.train's names as [P] tensors (the statistics float64 copies of `stats`; explained_variance and std
        float32-derived), per member."""
        self._refuse("PopulationA2C.train", unsupported)
        T = T or self.cfg.n_steps
        self._update(T)
        return self._train_stats(T)

    def _iteration(self, T: int):
        """One iteration's device work: rollout, GAE, update, repack"""
        self.collect_rollouts(T)
        self.compute_gae(T)
        self._update(T)

    def _replay_iteration(self, T: int):
        """_iteration as one replay of a HIP graph captured on one stream (a linear graph), captured when there is none
        for this key (PopulationPPO._iteration_graph_key; the capture launches nothing: the first iteration is a replay
        too).  The kernels read step_base, the table, the parameters and the optimiser state on the device when they run:
        set_hyper and copy_member between replays are stream-ordered writes into buffers the graph already addresses."""
        key = self._iteration_graph_key(T)
        if self._graph is None or self._graph_key != key:
            s = torch.cuda.Stream(device=self.env.device)
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s), torch.no_grad():
                self._iteration(T)
            self._graph, self._graph_key = g, key
        self._graph.replay()

    def learn(self, iterations: int, n_steps: Optional[int] = None, use_graph: bool = False, **unsupported):
        """`iterations` x (collect_rollouts, compute_gae, train) after an env reset; train()'s values per iteration, with
        mean_reward [P].  use_graph=True replays each iteration's device work as one HIP graph (_replay_iteration) and
        reads the statistics outside it, from the persistent buffers; the same bits as use_graph=False.
        self.control_test as PopulationPPO.learn's: its evaluations run before the iteration's device work, outside the
        capture, and the entry gains the transfer_* values."""
        self._refuse("PopulationA2C.learn", unsupported)
        T, P, epp = n_steps or self.cfg.n_steps, self.n_members, self.envs_per_member
        assert T <= self.cfg.n_steps
        control_test = self.control_test
        pushes = _control_test_plan(self, control_test, iterations, T)
        self._pbt_check()
        self.env.reset()
        hist = []
        for it in range(iterations):
            if pushes is not None and pushes[it]:
                control_test.evaluate(pushes[it])
            source = self._pbt_step(it, hist)
            if use_graph:
                self._replay_iteration(T)
            else:
                self._iteration(T)
            st = self._train_stats(T)
            st["mean_reward"] = self.rew_buf[:T].reshape(T, P, epp).mean(dim=(0, 2))
            if pushes is not None:
                st.update(control_test.history_entry())
            if source is not None:
                st["pbt_source"] = source
            hist.append(st)
        return hist

    # (exploit and explore: this class's key set and state rows; its update always reads the table on the device)
    _HYPER_KEYS = A2C_HYPER_COLUMN
    _check_value = staticmethod(_check_a2c_hyper_value)
    PBT_EXPLORE = A2C_PBT_EXPLORE

    def _table_on_device(self) -> bool:
        return True

    def _state_rows(self):
        """The two optimiser state rows (upd_s0, upd_s1): they travel together with the optimiser column"""
        return self.upd_s0, self.upd_s1

    def _fresh_state(self, p: int):
        """Member p's optimiser state as a new optimiser object has it: stream-ordered fills"""
        self.upd_s0[p].fill_(1.0 if self.optimizers[p] == "rmsprop_tf" else 0.0)
        self.upd_s1[p].zero_()
        self.upd_t[p].zero_()

    def set_hyper(self, p: int, **kw):
        """PopulationPPO.set_hyper for this class's keys (a2c_hyper_table's, validated the same way; nothing is written
        before every value has passed).  Naming an `optimizer` other than the member's present one also re-initialises
        that member's optimiser state and step count (upd_s0[p] ones for "rmsprop_tf", else zeros; upd_s1[p] and
        upd_t[p] 0) with stream-ordered fills -- what a new optimiser object starts from."""
        self._need_hyper("set_hyper", p)
        if getattr(self, "_hyper_stale", False):
            self.sync_hyper()
        unknown = sorted(set(kw) - set(A2C_HYPER_COLUMN))
        if unknown:
            raise ValueError(f"PopulationA2C.set_hyper: unknown key(s) {unknown}; a member's own values are "
                             f"{sorted(A2C_HYPER_COLUMN)}")
        new = {k: _check_a2c_hyper_value(k, x, f"PopulationA2C.set_hyper: member {p}") for k, x in kw.items()}
        col = A2C_HYPER_COLUMN["optimizer"]
        changed = "optimizer" in new and new["optimizer"] != float(self.hyper[p, col])
        for k, x in new.items():
            self.hyper[p, A2C_HYPER_COLUMN[k]] = x
        self.learning_rates[p] = float(self.hyper[p, A2C_HYPER_COLUMN["learning_rate"]])
        self._lr[p] = self.learning_rates[p]
        self.hyper_dev[p].copy_(self.hyper[p], non_blocking=True)
        if changed:
            self._fresh_state(p)

    def copy_member(self, src: int, dst: int, hyper: bool = True):
        """PopulationPPO.copy_member with this class's state: member src's parameters (the whole stride of flat), both
        optimiser state rows and the step count onto member dst, and with `hyper` its table row too (the optimiser kind
        among its columns: without it the state rows are read by dst's own optimiser)."""
        self._need_hyper("copy_member", src, dst)
        if getattr(self, "_hyper_stale", False):
            self.sync_hyper()
        if int(src) == int(dst):
            return
        for x in (self.flat, self.upd_s0, self.upd_s1, self.upd_t):
            x[dst].copy_(x[src])
        if hyper:
            self.hyper[dst] = self.hyper[src]
            self.learning_rates[dst] = self.learning_rates[src]
            self._lr[dst] = self._lr[src]
            self.hyper_dev[dst].copy_(self.hyper_dev[src])


def control_test_pushes(iterations: int, T: int, log_interval: int) -> list:
    """How often iteration it = 0 .. iterations - 1 of T rollout steps makes the reference's ControlTestCallback fly
    its step tests: (it + 1) * T // L - it * T // L, the multiples of L = log_interval among the callback's n_calls
    it * T + 1 .. (it + 1) * T (neural/callbacks.py:106).  ValueError for more than 256 in one iteration
    (b747_ppo_track_best's limit on one call's pushes)."""
    T, L = int(T), int(log_interval)
    if T < 1 or L < 1:
        raise ValueError(f"control_test_pushes: {T} rollout steps, log_interval {L} (both at least 1)")
    ms = [(it + 1) * T // L - it * T // L for it in range(int(iterations))]
    if ms and max(ms) > 256:
        raise ValueError(f"learn(control_test=...): {max(ms)} evaluations in one iteration ({T} rollout steps at "
                         f"log_interval {L}); b747_ppo_track_best takes at most 256 pushes a call -- raise log_interval")
    return ms


class ControlTest:
    """The reference's ControlTestCallback (neural/callbacks.py:46-120) kept on the device, for a PopulationPPO or a
    PPO(fused=True) (handled as one member, its `flat` seen as [1, stride]); DESIGN.md 19.

    The callback flies the step tests with the current deterministic policy every log_interval calls, appends the means
    over the references to three windows of the last window_length evaluations, logs the windowed means as
    transfer_custom/* and saves the model whenever the windowed mean quality beats the best so far; optimize() ranks a
    trial by that windowed quality and reloads the saved model (neural/agent.py:115-133).  Here evaluate() is a reset of
    ONE persistent test env, one evaluation launch that reads the learner's packed `flat` where it lies
    (b747_eval_population; b747_eval_episodes for a PPO) and one b747_ppo_track_best launch that keeps the books for
    every member: no host read, no synchronisation and no allocation after construction, so learn(control_test=...)
    stays free of host reads.

    The test env is population_step_tests' (PPO.step_tests' for a PPO): (P - 1) * 64 + R envs, the references repeated
    per 64-env group, the learner's env settings (_step_test_kwargs) overridden by env_kwargs (e.g. aero_err for
    main.py's test env), auto_reset off, tk the learner env's unless given.  State, all on the device: eval_out [7, n]
    (the last evaluation's per-env metrics), ring [3, P, W], count [P], last and window_mean [P, 3] (settling_time,
    overshoot, quality; NaN until the first evaluation), best_quality [P] (0 at first, as the callback's), best_eval [P]
    (the push that saved last; -1: nothing saved yet) and best_flat [P, stride] (a copy of the learner's flat at
    construction, so that it always holds a flyable policy)."""

    def __init__(self, learner, vartheta_ref, state0=(0, 11000, 250, 0, 0, 0), log_interval: int = 1000,
                 window_length: int = 30, tk: Optional[float] = None, **env_kwargs):
        from .ctrl_env import CtrlType
        refs = [float(v) for v in vartheta_ref] if isinstance(vartheta_ref, (list, tuple)) else [float(vartheta_ref)]
        R, W, L = len(refs), int(window_length), int(log_interval)
        if not 1 <= R <= 64:
            raise ValueError(f"ControlTest: {R} references (1 .. 64: one 64-env group per member)")
        if not 1 <= W <= 128:
            raise ValueError(f"ControlTest: window_length={W} (1 .. 128: b747_ppo_track_best keeps NumPy's summation "
                             "order up to 128 values)")
        if L < 1:
            raise ValueError(f"ControlTest: log_interval={L} (at least 1)")
        population = isinstance(learner, PopulationPPO)
        if not population and not (isinstance(learner, PPO) and learner.fused):
            raise ValueError("ControlTest: the learner is a PopulationPPO or a PPO(fused=True) (the evaluation reads "
                             "the packed parameter buffer `flat`)")
        self.learner, self.population = learner, population
        self.vartheta_ref, self.log_interval, self.window_length = refs, L, W
        P = learner.n_members if population else 1
        self.n_members, self.n_refs = P, R
        e = learner.env
        if e.obs_dim not in (3, 5):
            raise ValueError("ControlTest: the evaluation kernel runs a policy with a PID_LIKE or SPEED_MODE observation")
        kw = _step_test_kwargs(e) | env_kwargs
        kw["auto_reset"] = False
        ctrl_type = kw.pop("ctrl_type", CtrlType.MANUAL)
        self.tk = float(e.tk if tk is None else tk)
        dev, f64 = e.device, torch.float64
        n = (P - 1) * 64 + R
        env = BatchControllerEnv(n, kw.pop("observation_type"), kw.pop("reward_type"), kw.pop("norm_obs"),
                                 kw.pop("norm_act"), ctrl_type, kw.pop("ctrl_mode"), reset_ref_mode=None, tk=self.tk, **kw)
        env.set_state0(torch.tensor(state0, dtype=f64))
        env.set_reference(vartheta=torch.tensor((refs * 64)[:64] * P, dtype=f64, device=dev)[:n])
        self.env = env
        self.steps = int(math.ceil(self.tk / env.sample_time - 1e-9))
        self.vref = env.ref[0].to(f64).clone()
        self.y_base = self.vref * 180 / math.pi          # (the step tests' expression: the same bits)
        self.stride = int(learner.flat.numel() // P)
        self.eval_out = torch.zeros(len(learner._lib.EVAL_ROWS), n, dtype=f64, device=dev)
        nan = lambda *s: torch.full(s, math.nan, dtype=f64, device=dev)
        self.ring, self.last, self.window_mean = nan(3, P, W), nan(P, 3), nan(P, 3)
        self.count = torch.zeros(P, dtype=torch.int64, device=dev)
        self.best_quality = torch.zeros(P, dtype=f64, device=dev)
        self.best_eval = torch.full((P,), -1, dtype=torch.int64, device=dev)
        self.best_flat = learner.flat.detach().reshape(P, self.stride).clone()
        self.evaluations = 0          # evaluate() calls so far (host side; the device's count is pushes)

    def _reset_test_env(self):
        """The test env back to what a freshly built one is before its evaluation.  b747_env_reset leaves three things
        behind that the evaluation reads: the episode counter (it keys the reset's disturbance draws; a fresh env
        evaluates its episode 1), and tp and h_zh, which a reset does not rewrite (the TF_REFERENCE reward and the CS
        loop read them).  Three fills and the reset, all stream-ordered."""
        env = self.env
        env.episode.fill_(1)
        env.tp.zero_()
        env.h_zh.fill_(11000.0)
        env.reset()

    @torch.no_grad()
    def evaluate(self, repeat: int = 1):
        """One callback evaluation of the learner's current policies, booked `repeat` times (1 .. 256): the test env's
        reset, the evaluation launch on the learner's `flat` itself (packed after every update) and
        b747_ppo_track_best, on the current stream."""
        repeat = int(repeat)
        if not 1 <= repeat <= 256:
            raise ValueError(f"ControlTest.evaluate: repeat={repeat} (1 .. 256)")
        lr, env, p = self.learner, self.env, _p
        self._reset_test_env()
        if self.population:
            env.eval_population(self.steps, lr.flat, 64, signal="state_vartheta", scale=180 / math.pi,
                                y_base=self.y_base, out=self.eval_out)
        else:
            env.eval_episodes(self.steps, lr.flat, "state_vartheta", scale=180 / math.pi, y_base=self.y_base,
                              out=self.eval_out)
        lr._lib.check(lr._L.b747_ppo_track_best(
            p(self.eval_out), env.n, p(self.vref), self.tk, self.n_members, 64, self.n_refs, self.window_length, repeat,
            p(lr.flat), self.stride, p(self.ring), p(self.count), p(self.last), p(self.window_mean),
            p(self.best_quality), p(self.best_eval), p(self.best_flat), torch.cuda.current_stream().cuda_stream),
            "b747_ppo_track_best")
        self.evaluations += 1

    def history_entry(self) -> dict:
        """The callback's transfer_custom/* log values: [P] device clones of the windowed means (NaN before the first
        evaluation)"""
        wm = self.window_mean
        return {"transfer_settling_time": wm[:, 0].clone(), "transfer_overshoot": wm[:, 1].clone(),
                "transfer_quality": wm[:, 2].clone()}

    def objective(self) -> torch.Tensor:
        """[P] the windowed mean quality: what optimize()'s objective returns for a trial (neural/agent.py:131)"""
        return self.window_mean[:, 2]

    def best_member(self) -> torch.Tensor:
        """The member whose saved model reached the highest windowed quality (a device scalar)"""
        return self.best_quality.argmax()

    def best(self, p: int = 0) -> ActorCritic:
        """Member p's saved model (the callback's best_model file) as an ActorCritic on the learner's device; before the
        first save, the policy the member started with"""
        net = ActorCritic(self.learner.env.obs_dim).to(self.learner.env.device)
        load_flat(net, self.best_flat[int(p)])
        return net


def _control_test_plan(learner, control_test, iterations: int, T: int):
    """learn()'s pushes per iteration for its control_test (None: no evaluations)"""
    if control_test is None:
        return None
    if getattr(control_test, "learner", None) is not learner:
        raise ValueError("learn(control_test=...): the ControlTest was built for another learner")
    return control_test_pushes(iterations, T, control_test.log_interval)
