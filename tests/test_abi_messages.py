"""The argument validation of the policy, PPO and evaluation entry points, message by message: for every check of
b747_policy_act, b747_policy_pack_batch, b747_ppo_grad, b747_ppo_adam, b747_ppo_epoch, b747_ppo_epoch_population,
b747_ppo_epoch_batched, b747_ppo_rollout_lanes, b747_ppo_rollout_population, b747_eval_episodes and
b747_eval_population one call that fails it, the return code and the complete b747_last_error() bytes against the
literal table EXPECTED below; calls that fail two checks pin the order of the checks (the first one's message), and
the empty-batch cases pin which entry point looks at its pointers before it returns 0.

EXPECTED is a recording: `B747_LIB_PATH=<a libb747.so> python tests/test_abi_messages.py` prints the table that
library gives.  The one below was printed by the library as it stood before the entry points shared their validators
and pasted in unchanged; it is regenerated only when a message is changed on purpose, never from the code under test
to make this test pass.

No launch, no GPU (as tests/test_ppo_epoch_batched_abi.py): every pointer is a fake address that a launch would fault
on, so every call here is refused, or returns 0 before it would launch (an empty batch, no policies)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ppo_rollout_lanes_abi import OBS_MODEL_STATE, OBS_SPEED_MODE, _env   # noqa: E402  (the env descriptor)

F = 0x1000          # a fake address
NUM3 = 18952        # b747_policy_num_params(3), asserted below


def _batched_ws(od, batch):
    n_wg = min(256, -(-(-(-batch // 32)) // 2))
    return -(-(1024 + 72 * n_wg + 4 * (128 * od + 8579) * (n_wg + 1)) // 16) * 16


# entry point -> its arguments in order with the values of a call that every check accepts ("env": see _call)
UPD = dict(obs=F, act=F, old_logp=F, adv=F, ret=F)
LOSS = dict(clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-5)
ROLL = dict(obs_buf=F, act_buf=F, logp_buf=F, val_buf=F, rew_buf=F, done_buf=F)
EVAL = dict(n_env_steps=10, sig_row=0, scale=1.0, y_base=F, error_band=0.05, act_lo=-1.0, act_hi=1.0, eval_out=F)
CALLS = {
    "b747_policy_act": dict(params=F, obs_dim=3, n=64, obs=F, noise=None, seed=1, step_base=None, step=0, env_offset=0,
                            obs_out=F, act_out=F, logp_out=F, value_out=F, env_action=F, act_lo=-1.0, act_hi=1.0,
                            stream=None),
    "b747_policy_pack_batch": dict(params=F, obs_dim=3, n_policies=3, policy_stride=NUM3, stream=None),
    "b747_ppo_grad": dict(theta=F, obs_dim=3, **UPD, idx=F, batch=256, **LOSS, workspace=F, grad=F, stats=F, stream=None),
    "b747_ppo_adam": dict(theta=F, m=F, v=F, t=F, grad=F, n_params=8963, grad_scale=1.0, max_grad_norm=0.5, lr=3e-4,
                          **ADAM, stream=None),
    "b747_ppo_epoch": dict(theta=F, obs_dim=3, **UPD, perm=F, n_rows=896, batch_size=256, **LOSS, workspace=F, grad=F,
                           m=F, v=F, t=F, max_grad_norm=0.5, lr=3e-4, **ADAM, stats=F, stream=None),
    "b747_ppo_epoch_population": dict(theta=F, n_policies=3, policy_stride=NUM3, obs_dim=3, **UPD, perm=F, n_rows=896,
                                      batch_size=256, **LOSS, workspace=F, grad=F, m=F, v=F, t=F, max_grad_norm=0.5,
                                      lr="host", **ADAM, stats=F, stream=None),
    "b747_ppo_epoch_batched": dict(theta=F, n_policies=3, policy_stride=NUM3, obs_dim=3, **UPD, perm=F, n_rows=896,
                                   batch_size=256, **LOSS, workspace=F, workspace_bytes=3 * _batched_ws(3, 256), m=F, v=F,
                                   t=F, max_grad_norm=0.5, lr_dev=F, **ADAM, stats=F, stream=None),
    "b747_ppo_rollout": dict(env={}, params=F, seed=1, step_base=F, T=16, **ROLL, act_lo=-1.0, act_hi=1.0, stream=None),
    "b747_ppo_rollout_lanes": dict(env={}, params=F, seed=1, step_base=F, T=16, **ROLL, act_lo=-1.0, act_hi=1.0,
                                   stream=None),
    "b747_ppo_rollout_population": dict(env=dict(n=192), params=F, n_policies=3, policy_stride=NUM3, envs_per_policy=64,
                                        rew_pop=None, seed=1, step_base=F, T=16, **ROLL, last_val=F, act_lo=-1.0,
                                        act_hi=1.0, stream=None),
    "b747_eval_episodes": dict(env={}, params=F, **EVAL, stream=None),
    "b747_eval_population": dict(env=dict(n=192), params=F, n_policies=3, policy_stride=NUM3, envs_per_policy=64,
                                 pid_ss=None, pid_cs=None, **EVAL, stream=None),
}
NO_ENV, NO_CFG = dict(b=None), dict(cfg=None)
# env keys beside test_ppo_rollout_lanes_abi._env's own: b / cfg (None: a NULL structure), auto_reset, action, and
# c = None (NULL constants)


def _nulls(*names):
    return [(n, {n: None}) for n in names]


ROLL_CASES = _nulls("params", *ROLL) + [
    ("no_batch", dict(env=NO_ENV)), ("no_config", dict(env=NO_CFG)), ("n_negative", dict(env=dict(n=-1))),
    ("consts", dict(env=dict(c=None))), ("T", dict(T=-1)), ("act_range", dict(act_lo=0.5, act_hi=-0.5)),
    ("act_nan", dict(act_lo=float("nan"))),
    ("obs_dim_7", dict(env=dict(obs_type=OBS_MODEL_STATE))), ("fp32_state", dict(env=dict(x_f64=0))),
    ("recording", dict(env=dict(sig=F))),
    # order: the first failing check speaks
    ("consts+act_range", dict(env=dict(c=None), act_lo=0.5, act_hi=-0.5)), ("params+T", dict(params=None, T=-1)),
    ("done_buf+fp32_state", dict(done_buf=None, env=dict(x_f64=0))), ("T+obs_dim_7", dict(T=-1, env=dict(obs_type=OBS_MODEL_STATE))),
    ("n_negative+params", dict(env=dict(n=-1), params=None)),
]
TILING_CASES = [
    ("envs_per_policy_0", dict(envs_per_policy=0)), ("envs_per_policy_100", dict(envs_per_policy=100)),
    ("n_policies_0", dict(n_policies=0)), ("n_below", dict(env=dict(n=128))), ("n_above", dict(env=dict(n=193))),
    ("stride_short", dict(policy_stride=NUM3 - 4)), ("stride_odd", dict(policy_stride=NUM3 + 2)),
    ("envs_per_policy+stride", dict(envs_per_policy=0, policy_stride=0)), ("n_policies+n", dict(n_policies=0, env=dict(n=128))),
    ("n+stride", dict(env=dict(n=128), policy_stride=0)),
]
EVAL_CASES = _nulls("y_base", "eval_out") + [
    ("no_batch", dict(env=NO_ENV)), ("consts", dict(env=dict(c=None))), ("steps", dict(n_env_steps=-1)),
    ("sig_row_negative", dict(sig_row=-1)), ("sig_row_31", dict(sig_row=31)), ("act_range", dict(act_lo=0.5, act_hi=-0.5)),
    ("fp32_state", dict(env=dict(x_f64=0))), ("auto_reset", dict(env=dict(auto_reset=1))),
    ("obs_dim_7", dict(env=dict(obs_type=OBS_MODEL_STATE))), ("action", dict(params=None, n_policies=0, env=dict(action=None))),
    ("empty_batch", dict(env=dict(n=0, c=None), y_base=None)),        # returns at the env check's 0
    ("consts+action", dict(env=dict(c=None, action=None), params=None, n_policies=0)),
    ("y_base+fp32_state", dict(y_base=None, env=dict(x_f64=0))), ("act_range+auto_reset", dict(act_lo=1.0, act_hi=0.0, env=dict(auto_reset=1))),
    ("fp32_state+action", dict(env=dict(x_f64=0, action=None), params=None, n_policies=0)),
]
UPD_NULLS = ("theta", "obs", "act", "old_logp", "adv", "ret")
EPOCH_CASES = [("obs_dim_4", dict(obs_dim=4)), ("obs_dim_11", dict(obs_dim=11)), ("n_rows", dict(n_rows=1)),
               ("batch_size", dict(batch_size=1)), ("tail_of_one", dict(n_rows=1025, batch_size=64)),
               ("theta+stats", dict(theta=None, stats=None)), ("obs_dim+stats", dict(obs_dim=4, stats=None)),
               ("ret+perm", dict(ret=None, perm=None)), ("perm+n_rows", dict(perm=None, n_rows=1)),
               ("n_rows+batch_size", dict(n_rows=1, batch_size=1)), ("batch_size+workspace", dict(batch_size=1, workspace=None)),
               ("workspace+t", dict(workspace=None, t=None)), ("m+v", dict(m=None, v=None)), ("t+stats", dict(t=None, stats=None))]
MEMBER_CASES = [("n_policies_0", dict(n_policies=0)), ("n_policies_negative", dict(n_policies=-2)),
                ("stride_0", dict(policy_stride=0)), ("stride_short", dict(policy_stride=NUM3 - 4)),
                ("stride_odd", dict(policy_stride=NUM3 + 2)), ("obs_dim+n_policies", dict(obs_dim=4, n_policies=0)),
                ("n_policies+stride", dict(n_policies=0, policy_stride=0)), ("stride+obs", dict(policy_stride=0, obs=None))]
CASES = {
    "b747_policy_act": [
        ("n_negative", dict(n=-1))] + _nulls("params", "obs", "act_out", "logp_out", "value_out", "env_action") + [
        ("act_range", dict(act_lo=0.5, act_hi=-0.5)), ("act_nan", dict(act_hi=float("nan"))),
        ("obs_dim_4", dict(obs_dim=4)), ("obs_dim_11", dict(obs_dim=11)), ("obs_dim_0", dict(obs_dim=0)),
        ("empty_batch", dict(n=0, params=None, obs_dim=4)),
        ("n_negative+obs_dim", dict(n=-1, obs_dim=4)), ("params+obs_dim", dict(params=None, obs_dim=4)),
        ("act_range+obs_dim", dict(act_lo=0.5, act_hi=-0.5, obs_dim=4)), ("params+act_range", dict(params=None, act_lo=1.0, act_hi=0.0))],
    "b747_policy_pack_batch": _nulls("params") + [
        ("obs_dim_0", dict(obs_dim=0)), ("obs_dim_11", dict(obs_dim=11)), ("n_policies_negative", dict(n_policies=-1)),
        ("n_policies_65536", dict(n_policies=65536)), ("stride_short", dict(policy_stride=NUM3 - 4)),
        ("stride_odd", dict(policy_stride=NUM3 + 2)), ("no_policies", dict(n_policies=0)),
        ("params+stride", dict(params=None, policy_stride=0)), ("obs_dim+stride", dict(obs_dim=0, policy_stride=0)),
        ("n_policies+stride", dict(n_policies=-1, policy_stride=0))],
    "b747_ppo_grad": _nulls(*UPD_NULLS, "idx", "workspace", "grad", "stats") + [
        ("obs_dim_4", dict(obs_dim=4)), ("obs_dim_11", dict(obs_dim=11)), ("batch_1", dict(batch=1)),
        ("theta+stats", dict(theta=None, stats=None)), ("obs_dim+stats", dict(obs_dim=4, stats=None)),
        ("idx+batch", dict(idx=None, batch=1)), ("batch+workspace", dict(batch=0, workspace=None)),
        ("workspace+grad", dict(workspace=None, grad=None)), ("grad+stats", dict(grad=None, stats=None))],
    "b747_ppo_adam": _nulls("theta", "m", "v", "t", "grad") + [
        ("n_params_0", dict(n_params=0)), ("theta+n_params", dict(theta=None, n_params=0)),
        ("m+grad", dict(m=None, grad=None)), ("grad+n_params", dict(grad=None, n_params=0))],
    "b747_ppo_epoch": _nulls(*UPD_NULLS, "perm", "workspace", "grad", "m", "v", "t", "stats") + EPOCH_CASES + [
        ("grad+m", dict(grad=None, m=None))],
    "b747_ppo_epoch_population": _nulls(*UPD_NULLS, "perm", "workspace", "grad", "m", "v", "t", "lr", "stats")
    + EPOCH_CASES + MEMBER_CASES + [("grad+m", dict(grad=None, m=None)), ("t+lr", dict(t=None, lr=None)),
                                    ("lr+stats", dict(lr=None, stats=None))],
    "b747_ppo_epoch_batched": _nulls(*UPD_NULLS, "perm", "workspace", "m", "v", "t", "lr_dev", "stats")
    + EPOCH_CASES + MEMBER_CASES + [
        ("workspace_bytes_0", dict(workspace_bytes=0)), ("workspace_bytes_negative", dict(workspace_bytes=-16)),
        ("workspace_bytes_one_short", dict(workspace_bytes=_batched_ws(3, 256) - 1)),
        ("workspace+workspace_bytes", dict(workspace=None, workspace_bytes=0)),
        ("workspace_bytes+m", dict(workspace_bytes=0, m=None)), ("t+lr_dev", dict(t=None, lr_dev=None)),
        ("lr_dev+stats", dict(lr_dev=None, stats=None))],
    "b747_ppo_rollout": [("empty_batch", dict(env=dict(n=0, c=None), params=None, T=-1))],   # at the env check's 0
    "b747_ppo_rollout_lanes": ROLL_CASES + [
        ("empty_batch", dict(env=dict(n=0))),                                 # 0, but only after the pointers
        ("empty_batch+params", dict(env=dict(n=0), params=None)), ("empty_batch+T", dict(env=dict(n=0), T=-1)),
        ("empty_batch+fp32_state", dict(env=dict(n=0, x_f64=0)))],
    "b747_ppo_rollout_population": ROLL_CASES + TILING_CASES + [
        ("empty_batch", dict(env=dict(n=0))),                                 # refused: no group
        ("empty_batch+params", dict(env=dict(n=0), params=None)),
        ("empty_batch+envs_per_policy", dict(env=dict(n=0), envs_per_policy=0)),
        ("empty_batch+stride", dict(env=dict(n=0), policy_stride=0)),
        ("act_range+envs_per_policy", dict(act_lo=1.0, act_hi=0.0, envs_per_policy=0)),
        ("n_policies+obs_dim_7", dict(n_policies=0, env=dict(obs_type=OBS_MODEL_STATE))),
        ("recording+n", dict(env=dict(sig=F, n=128))), ("obs_dim_5_stride_of_3", dict(env=dict(obs_type=OBS_SPEED_MODE, n=192)))],
    "b747_eval_episodes": EVAL_CASES,
    "b747_eval_population": EVAL_CASES + TILING_CASES + [
        ("n_policies_without_params", dict(params=None, n_policies=1)),
        ("action+n_policies", dict(params=None, n_policies=1, env=dict(action=None))),
        ("auto_reset+envs_per_policy", dict(env=dict(auto_reset=1), envs_per_policy=0)),
        ("obs_dim_5_stride_of_3", dict(env=dict(obs_type=OBS_SPEED_MODE, n=192)))],
}

EXPECTED = {
    'b747_policy_act/n_negative': (-1, b'invalid argument: n < 0'),
    'b747_policy_act/params': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/obs': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/act_out': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/logp_out': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/value_out': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/env_action': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/act_range': (-1, b'invalid argument: act_lo > act_hi'),
    'b747_policy_act/act_nan': (-1, b'invalid argument: act_lo > act_hi'),
    'b747_policy_act/obs_dim_4': (-1, b'invalid argument: obs_dim (PID_LIKE 3, SPEED_MODE 5, MODEL_STATE 7, PID_AERO 8, PID_SPEED_AERO 10)'),
    'b747_policy_act/obs_dim_11': (-1, b'invalid argument: obs_dim (PID_LIKE 3, SPEED_MODE 5, MODEL_STATE 7, PID_AERO 8, PID_SPEED_AERO 10)'),
    'b747_policy_act/obs_dim_0': (-1, b'invalid argument: obs_dim (PID_LIKE 3, SPEED_MODE 5, MODEL_STATE 7, PID_AERO 8, PID_SPEED_AERO 10)'),
    'b747_policy_act/empty_batch': (0, b''),
    'b747_policy_act/n_negative+obs_dim': (-1, b'invalid argument: n < 0'),
    'b747_policy_act/params+obs_dim': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_act/act_range+obs_dim': (-1, b'invalid argument: act_lo > act_hi'),
    'b747_policy_act/params+act_range': (-1, b'invalid argument: NULL buffer'),
    'b747_policy_pack_batch/params': (-1, b'invalid argument: b747_policy_pack_batch: params is NULL'),
    'b747_policy_pack_batch/obs_dim_0': (-1, b'invalid argument: b747_policy_pack_batch: obs_dim'),
    'b747_policy_pack_batch/obs_dim_11': (-1, b'invalid argument: b747_policy_pack_batch: obs_dim'),
    'b747_policy_pack_batch/n_policies_negative': (-1, b'invalid argument: b747_policy_pack_batch: n_policies (0 .. 65535)'),
    'b747_policy_pack_batch/n_policies_65536': (-1, b'invalid argument: b747_policy_pack_batch: n_policies (0 .. 65535)'),
    'b747_policy_pack_batch/stride_short': (-1, b'invalid argument: b747_policy_pack_batch: policy_stride (at least b747_policy_num_params floats, a multiple of 4)'),
    'b747_policy_pack_batch/stride_odd': (-1, b'invalid argument: b747_policy_pack_batch: policy_stride (at least b747_policy_num_params floats, a multiple of 4)'),
    'b747_policy_pack_batch/no_policies': (0, b''),
    'b747_policy_pack_batch/params+stride': (-1, b'invalid argument: b747_policy_pack_batch: params is NULL'),
    'b747_policy_pack_batch/obs_dim+stride': (-1, b'invalid argument: b747_policy_pack_batch: obs_dim'),
    'b747_policy_pack_batch/n_policies+stride': (-1, b'invalid argument: b747_policy_pack_batch: n_policies (0 .. 65535)'),
    'b747_ppo_grad/theta': (-1, b'invalid argument: theta is NULL'),
    'b747_ppo_grad/obs': (-1, b'invalid argument: obs is NULL'),
    'b747_ppo_grad/act': (-1, b'invalid argument: act is NULL'),
    'b747_ppo_grad/old_logp': (-1, b'invalid argument: old_logp is NULL'),
    'b747_ppo_grad/adv': (-1, b'invalid argument: adv is NULL'),
    'b747_ppo_grad/ret': (-1, b'invalid argument: ret is NULL'),
    'b747_ppo_grad/idx': (-1, b'invalid argument: idx is NULL'),
    'b747_ppo_grad/workspace': (-1, b'invalid argument: workspace is NULL'),
    'b747_ppo_grad/grad': (-1, b'invalid argument: grad is NULL'),
    'b747_ppo_grad/stats': (-1, b'invalid argument: stats is NULL'),
    'b747_ppo_grad/obs_dim_4': (-1, b'invalid argument: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_grad/obs_dim_11': (-1, b'invalid argument: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_grad/batch_1': (-1, b"invalid argument: batch < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_grad/theta+stats': (-1, b'invalid argument: theta is NULL'),
    'b747_ppo_grad/obs_dim+stats': (-1, b'invalid argument: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_grad/idx+batch': (-1, b'invalid argument: idx is NULL'),
    'b747_ppo_grad/batch+workspace': (-1, b"invalid argument: batch < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_grad/workspace+grad': (-1, b'invalid argument: workspace is NULL'),
    'b747_ppo_grad/grad+stats': (-1, b'invalid argument: grad is NULL'),
    'b747_ppo_adam/theta': (-1, b'invalid argument: theta is NULL'),
    'b747_ppo_adam/m': (-1, b'invalid argument: m is NULL'),
    'b747_ppo_adam/v': (-1, b'invalid argument: v is NULL'),
    'b747_ppo_adam/t': (-1, b'invalid argument: t is NULL'),
    'b747_ppo_adam/grad': (-1, b'invalid argument: grad is NULL'),
    'b747_ppo_adam/n_params_0': (-1, b'invalid argument: n_params < 1'),
    'b747_ppo_adam/theta+n_params': (-1, b'invalid argument: theta is NULL'),
    'b747_ppo_adam/m+grad': (-1, b'invalid argument: m is NULL'),
    'b747_ppo_adam/grad+n_params': (-1, b'invalid argument: grad is NULL'),
    'b747_ppo_epoch/theta': (-1, b'invalid argument: theta is NULL'),
    'b747_ppo_epoch/obs': (-1, b'invalid argument: obs is NULL'),
    'b747_ppo_epoch/act': (-1, b'invalid argument: act is NULL'),
    'b747_ppo_epoch/old_logp': (-1, b'invalid argument: old_logp is NULL'),
    'b747_ppo_epoch/adv': (-1, b'invalid argument: adv is NULL'),
    'b747_ppo_epoch/ret': (-1, b'invalid argument: ret is NULL'),
    'b747_ppo_epoch/perm': (-1, b'invalid argument: perm is NULL'),
    'b747_ppo_epoch/workspace': (-1, b'invalid argument: workspace is NULL'),
    'b747_ppo_epoch/grad': (-1, b'invalid argument: grad is NULL'),
    'b747_ppo_epoch/m': (-1, b'invalid argument: m is NULL'),
    'b747_ppo_epoch/v': (-1, b'invalid argument: v is NULL'),
    'b747_ppo_epoch/t': (-1, b'invalid argument: t is NULL'),
    'b747_ppo_epoch/stats': (-1, b'invalid argument: stats is NULL'),
    'b747_ppo_epoch/obs_dim_4': (-1, b'invalid argument: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch/obs_dim_11': (-1, b'invalid argument: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch/n_rows': (-1, b"invalid argument: n_rows < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch/batch_size': (-1, b"invalid argument: batch_size < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch/tail_of_one': (-1, b'invalid argument: n_rows % batch_size == 1 (the last minibatch would be one row: no standard deviation)'),
    'b747_ppo_epoch/theta+stats': (-1, b'invalid argument: theta is NULL'),
    'b747_ppo_epoch/obs_dim+stats': (-1, b'invalid argument: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch/ret+perm': (-1, b'invalid argument: ret is NULL'),
    'b747_ppo_epoch/perm+n_rows': (-1, b'invalid argument: perm is NULL'),
    'b747_ppo_epoch/n_rows+batch_size': (-1, b"invalid argument: n_rows < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch/batch_size+workspace': (-1, b"invalid argument: batch_size < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch/workspace+t': (-1, b'invalid argument: workspace is NULL'),
    'b747_ppo_epoch/m+v': (-1, b'invalid argument: m is NULL'),
    'b747_ppo_epoch/t+stats': (-1, b'invalid argument: t is NULL'),
    'b747_ppo_epoch/grad+m': (-1, b'invalid argument: grad is NULL'),
    'b747_ppo_epoch_population/theta': (-1, b'invalid argument: b747_ppo_epoch_population: theta is NULL'),
    'b747_ppo_epoch_population/obs': (-1, b'invalid argument: b747_ppo_epoch_population: obs is NULL'),
    'b747_ppo_epoch_population/act': (-1, b'invalid argument: b747_ppo_epoch_population: act is NULL'),
    'b747_ppo_epoch_population/old_logp': (-1, b'invalid argument: b747_ppo_epoch_population: old_logp is NULL'),
    'b747_ppo_epoch_population/adv': (-1, b'invalid argument: b747_ppo_epoch_population: adv is NULL'),
    'b747_ppo_epoch_population/ret': (-1, b'invalid argument: b747_ppo_epoch_population: ret is NULL'),
    'b747_ppo_epoch_population/perm': (-1, b'invalid argument: b747_ppo_epoch_population: perm is NULL'),
    'b747_ppo_epoch_population/workspace': (-1, b'invalid argument: b747_ppo_epoch_population: workspace is NULL'),
    'b747_ppo_epoch_population/grad': (-1, b'invalid argument: b747_ppo_epoch_population: grad is NULL'),
    'b747_ppo_epoch_population/m': (-1, b'invalid argument: b747_ppo_epoch_population: m is NULL'),
    'b747_ppo_epoch_population/v': (-1, b'invalid argument: b747_ppo_epoch_population: v is NULL'),
    'b747_ppo_epoch_population/t': (-1, b'invalid argument: b747_ppo_epoch_population: t is NULL'),
    'b747_ppo_epoch_population/lr': (-1, b'invalid argument: b747_ppo_epoch_population: lr is NULL (a host array, one learning rate per member)'),
    'b747_ppo_epoch_population/stats': (-1, b'invalid argument: b747_ppo_epoch_population: stats is NULL'),
    'b747_ppo_epoch_population/obs_dim_4': (-1, b'invalid argument: b747_ppo_epoch_population: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_population/obs_dim_11': (-1, b'invalid argument: b747_ppo_epoch_population: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_population/n_rows': (-1, b"invalid argument: b747_ppo_epoch_population: n_rows < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_population/batch_size': (-1, b"invalid argument: b747_ppo_epoch_population: batch_size < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_population/tail_of_one': (-1, b'invalid argument: b747_ppo_epoch_population: n_rows % batch_size == 1 (the last minibatch would be one row: no standard deviation)'),
    'b747_ppo_epoch_population/theta+stats': (-1, b'invalid argument: b747_ppo_epoch_population: theta is NULL'),
    'b747_ppo_epoch_population/obs_dim+stats': (-1, b'invalid argument: b747_ppo_epoch_population: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_population/ret+perm': (-1, b'invalid argument: b747_ppo_epoch_population: ret is NULL'),
    'b747_ppo_epoch_population/perm+n_rows': (-1, b'invalid argument: b747_ppo_epoch_population: perm is NULL'),
    'b747_ppo_epoch_population/n_rows+batch_size': (-1, b"invalid argument: b747_ppo_epoch_population: n_rows < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_population/batch_size+workspace': (-1, b"invalid argument: b747_ppo_epoch_population: batch_size < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_population/workspace+t': (-1, b'invalid argument: b747_ppo_epoch_population: workspace is NULL'),
    'b747_ppo_epoch_population/m+v': (-1, b'invalid argument: b747_ppo_epoch_population: m is NULL'),
    'b747_ppo_epoch_population/t+stats': (-1, b'invalid argument: b747_ppo_epoch_population: t is NULL'),
    'b747_ppo_epoch_population/n_policies_0': (-1, b'invalid argument: b747_ppo_epoch_population: n_policies < 1'),
    'b747_ppo_epoch_population/n_policies_negative': (-1, b'invalid argument: b747_ppo_epoch_population: n_policies < 1'),
    'b747_ppo_epoch_population/stride_0': (-1, b'invalid argument: b747_ppo_epoch_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_population/stride_short': (-1, b'invalid argument: b747_ppo_epoch_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_population/stride_odd': (-1, b'invalid argument: b747_ppo_epoch_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_population/obs_dim+n_policies': (-1, b'invalid argument: b747_ppo_epoch_population: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_population/n_policies+stride': (-1, b'invalid argument: b747_ppo_epoch_population: n_policies < 1'),
    'b747_ppo_epoch_population/stride+obs': (-1, b'invalid argument: b747_ppo_epoch_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_population/grad+m': (-1, b'invalid argument: b747_ppo_epoch_population: grad is NULL'),
    'b747_ppo_epoch_population/t+lr': (-1, b'invalid argument: b747_ppo_epoch_population: t is NULL'),
    'b747_ppo_epoch_population/lr+stats': (-1, b'invalid argument: b747_ppo_epoch_population: lr is NULL (a host array, one learning rate per member)'),
    'b747_ppo_epoch_batched/theta': (-1, b'invalid argument: b747_ppo_epoch_batched: theta is NULL'),
    'b747_ppo_epoch_batched/obs': (-1, b'invalid argument: b747_ppo_epoch_batched: obs is NULL'),
    'b747_ppo_epoch_batched/act': (-1, b'invalid argument: b747_ppo_epoch_batched: act is NULL'),
    'b747_ppo_epoch_batched/old_logp': (-1, b'invalid argument: b747_ppo_epoch_batched: old_logp is NULL'),
    'b747_ppo_epoch_batched/adv': (-1, b'invalid argument: b747_ppo_epoch_batched: adv is NULL'),
    'b747_ppo_epoch_batched/ret': (-1, b'invalid argument: b747_ppo_epoch_batched: ret is NULL'),
    'b747_ppo_epoch_batched/perm': (-1, b'invalid argument: b747_ppo_epoch_batched: perm is NULL'),
    'b747_ppo_epoch_batched/workspace': (-1, b'invalid argument: b747_ppo_epoch_batched: workspace is NULL'),
    'b747_ppo_epoch_batched/m': (-1, b'invalid argument: b747_ppo_epoch_batched: m is NULL'),
    'b747_ppo_epoch_batched/v': (-1, b'invalid argument: b747_ppo_epoch_batched: v is NULL'),
    'b747_ppo_epoch_batched/t': (-1, b'invalid argument: b747_ppo_epoch_batched: t is NULL'),
    'b747_ppo_epoch_batched/lr_dev': (-1, b'invalid argument: b747_ppo_epoch_batched: lr_dev is NULL (a device array, one learning rate per member)'),
    'b747_ppo_epoch_batched/stats': (-1, b'invalid argument: b747_ppo_epoch_batched: stats is NULL'),
    'b747_ppo_epoch_batched/obs_dim_4': (-1, b'invalid argument: b747_ppo_epoch_batched: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_batched/obs_dim_11': (-1, b'invalid argument: b747_ppo_epoch_batched: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_batched/n_rows': (-1, b"invalid argument: b747_ppo_epoch_batched: n_rows < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_batched/batch_size': (-1, b"invalid argument: b747_ppo_epoch_batched: batch_size < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_batched/tail_of_one': (-1, b'invalid argument: b747_ppo_epoch_batched: n_rows % batch_size == 1 (the last minibatch would be one row: no standard deviation)'),
    'b747_ppo_epoch_batched/theta+stats': (-1, b'invalid argument: b747_ppo_epoch_batched: theta is NULL'),
    'b747_ppo_epoch_batched/obs_dim+stats': (-1, b'invalid argument: b747_ppo_epoch_batched: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_batched/ret+perm': (-1, b'invalid argument: b747_ppo_epoch_batched: ret is NULL'),
    'b747_ppo_epoch_batched/perm+n_rows': (-1, b'invalid argument: b747_ppo_epoch_batched: perm is NULL'),
    'b747_ppo_epoch_batched/n_rows+batch_size': (-1, b"invalid argument: b747_ppo_epoch_batched: n_rows < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_batched/batch_size+workspace': (-1, b"invalid argument: b747_ppo_epoch_batched: batch_size < 2 (the advantages' standard deviation needs two rows)"),
    'b747_ppo_epoch_batched/workspace+t': (-1, b'invalid argument: b747_ppo_epoch_batched: workspace is NULL'),
    'b747_ppo_epoch_batched/m+v': (-1, b'invalid argument: b747_ppo_epoch_batched: m is NULL'),
    'b747_ppo_epoch_batched/t+stats': (-1, b'invalid argument: b747_ppo_epoch_batched: t is NULL'),
    'b747_ppo_epoch_batched/n_policies_0': (-1, b'invalid argument: b747_ppo_epoch_batched: n_policies < 1'),
    'b747_ppo_epoch_batched/n_policies_negative': (-1, b'invalid argument: b747_ppo_epoch_batched: n_policies < 1'),
    'b747_ppo_epoch_batched/stride_0': (-1, b'invalid argument: b747_ppo_epoch_batched: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_batched/stride_short': (-1, b'invalid argument: b747_ppo_epoch_batched: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_batched/stride_odd': (-1, b'invalid argument: b747_ppo_epoch_batched: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_batched/obs_dim+n_policies': (-1, b'invalid argument: b747_ppo_epoch_batched: obs_dim (3, 5, 7, 8 or 10)'),
    'b747_ppo_epoch_batched/n_policies+stride': (-1, b'invalid argument: b747_ppo_epoch_batched: n_policies < 1'),
    'b747_ppo_epoch_batched/stride+obs': (-1, b'invalid argument: b747_ppo_epoch_batched: policy_stride (at least b747_policy_num_params floats and a multiple of 4)'),
    'b747_ppo_epoch_batched/workspace_bytes_0': (-1, b"invalid argument: b747_ppo_epoch_batched: workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch_size))"),
    'b747_ppo_epoch_batched/workspace_bytes_negative': (-1, b"invalid argument: b747_ppo_epoch_batched: workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch_size))"),
    'b747_ppo_epoch_batched/workspace_bytes_one_short': (-1, b"invalid argument: b747_ppo_epoch_batched: workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch_size))"),
    'b747_ppo_epoch_batched/workspace+workspace_bytes': (-1, b'invalid argument: b747_ppo_epoch_batched: workspace is NULL'),
    'b747_ppo_epoch_batched/workspace_bytes+m': (-1, b"invalid argument: b747_ppo_epoch_batched: workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch_size))"),
    'b747_ppo_epoch_batched/t+lr_dev': (-1, b'invalid argument: b747_ppo_epoch_batched: t is NULL'),
    'b747_ppo_epoch_batched/lr_dev+stats': (-1, b'invalid argument: b747_ppo_epoch_batched: lr_dev is NULL (a device array, one learning rate per member)'),
    'b747_ppo_rollout/empty_batch': (0, b''),
    'b747_ppo_rollout_lanes/params': (-1, b'invalid argument: b747_ppo_rollout_lanes: params is NULL'),
    'b747_ppo_rollout_lanes/obs_buf': (-1, b'invalid argument: b747_ppo_rollout_lanes: obs_buf is NULL'),
    'b747_ppo_rollout_lanes/act_buf': (-1, b'invalid argument: b747_ppo_rollout_lanes: act_buf is NULL'),
    'b747_ppo_rollout_lanes/logp_buf': (-1, b'invalid argument: b747_ppo_rollout_lanes: logp_buf is NULL'),
    'b747_ppo_rollout_lanes/val_buf': (-1, b'invalid argument: b747_ppo_rollout_lanes: val_buf is NULL'),
    'b747_ppo_rollout_lanes/rew_buf': (-1, b'invalid argument: b747_ppo_rollout_lanes: rew_buf is NULL'),
    'b747_ppo_rollout_lanes/done_buf': (-1, b'invalid argument: b747_ppo_rollout_lanes: done_buf is NULL'),
    'b747_ppo_rollout_lanes/no_batch': (-1, b'invalid argument: env batch/config is NULL'),
    'b747_ppo_rollout_lanes/no_config': (-1, b'invalid argument: env batch/config is NULL'),
    'b747_ppo_rollout_lanes/n_negative': (-1, b'invalid argument: n < 0'),
    'b747_ppo_rollout_lanes/consts': (-1, b'invalid argument: b747_ppo_rollout_lanes: consts is NULL'),
    'b747_ppo_rollout_lanes/T': (-1, b'invalid argument: b747_ppo_rollout_lanes: T < 0'),
    'b747_ppo_rollout_lanes/act_range': (-1, b'invalid argument: b747_ppo_rollout_lanes: act_lo > act_hi'),
    'b747_ppo_rollout_lanes/act_nan': (-1, b'invalid argument: b747_ppo_rollout_lanes: act_lo > act_hi'),
    'b747_ppo_rollout_lanes/obs_dim_7': (-1, b'invalid argument: b747_ppo_rollout_lanes: obs_dim (the one-wave rollout kernel runs a policy with PID_LIKE 3 or SPEED_MODE 5 only; use b747_policy_act + b747_env_step)'),
    'b747_ppo_rollout_lanes/fp32_state': (-1, b'invalid argument: b747_ppo_rollout_lanes: x_f64 (the one-wave rollout kernel keeps fp64 state only)'),
    'b747_ppo_rollout_lanes/recording': (-1, b'invalid argument: b747_ppo_rollout_lanes: sig (no per-DLL-step signal recording inside the rollout kernel)'),
    'b747_ppo_rollout_lanes/consts+act_range': (-1, b'invalid argument: b747_ppo_rollout_lanes: consts is NULL'),
    'b747_ppo_rollout_lanes/params+T': (-1, b'invalid argument: b747_ppo_rollout_lanes: params is NULL'),
    'b747_ppo_rollout_lanes/done_buf+fp32_state': (-1, b'invalid argument: b747_ppo_rollout_lanes: done_buf is NULL'),
    'b747_ppo_rollout_lanes/T+obs_dim_7': (-1, b'invalid argument: b747_ppo_rollout_lanes: T < 0'),
    'b747_ppo_rollout_lanes/n_negative+params': (-1, b'invalid argument: n < 0'),
    'b747_ppo_rollout_lanes/empty_batch': (0, b''),
    'b747_ppo_rollout_lanes/empty_batch+params': (-1, b'invalid argument: b747_ppo_rollout_lanes: params is NULL'),
    'b747_ppo_rollout_lanes/empty_batch+T': (-1, b'invalid argument: b747_ppo_rollout_lanes: T < 0'),
    'b747_ppo_rollout_lanes/empty_batch+fp32_state': (0, b''),
    'b747_ppo_rollout_population/params': (-1, b'invalid argument: b747_ppo_rollout_population: params is NULL'),
    'b747_ppo_rollout_population/obs_buf': (-1, b'invalid argument: b747_ppo_rollout_population: obs_buf is NULL'),
    'b747_ppo_rollout_population/act_buf': (-1, b'invalid argument: b747_ppo_rollout_population: act_buf is NULL'),
    'b747_ppo_rollout_population/logp_buf': (-1, b'invalid argument: b747_ppo_rollout_population: logp_buf is NULL'),
    'b747_ppo_rollout_population/val_buf': (-1, b'invalid argument: b747_ppo_rollout_population: val_buf is NULL'),
    'b747_ppo_rollout_population/rew_buf': (-1, b'invalid argument: b747_ppo_rollout_population: rew_buf is NULL'),
    'b747_ppo_rollout_population/done_buf': (-1, b'invalid argument: b747_ppo_rollout_population: done_buf is NULL'),
    'b747_ppo_rollout_population/no_batch': (-1, b'invalid argument: env batch/config is NULL'),
    'b747_ppo_rollout_population/no_config': (-1, b'invalid argument: env batch/config is NULL'),
    'b747_ppo_rollout_population/n_negative': (-1, b'invalid argument: n < 0'),
    'b747_ppo_rollout_population/consts': (-1, b'invalid argument: b747_ppo_rollout_population: consts is NULL'),
    'b747_ppo_rollout_population/T': (-1, b'invalid argument: b747_ppo_rollout_population: T < 0'),
    'b747_ppo_rollout_population/act_range': (-1, b'invalid argument: b747_ppo_rollout_population: act_lo > act_hi'),
    'b747_ppo_rollout_population/act_nan': (-1, b'invalid argument: b747_ppo_rollout_population: act_lo > act_hi'),
    'b747_ppo_rollout_population/obs_dim_7': (-1, b'invalid argument: b747_ppo_rollout_population: obs_dim (the one-wave rollout kernel runs a policy with PID_LIKE 3 or SPEED_MODE 5 only)'),
    'b747_ppo_rollout_population/fp32_state': (-1, b'invalid argument: b747_ppo_rollout_population: x_f64 (the one-wave rollout kernel keeps fp64 state only)'),
    'b747_ppo_rollout_population/recording': (-1, b'invalid argument: b747_ppo_rollout_population: sig (no per-DLL-step signal recording inside the rollout kernel)'),
    'b747_ppo_rollout_population/consts+act_range': (-1, b'invalid argument: b747_ppo_rollout_population: consts is NULL'),
    'b747_ppo_rollout_population/params+T': (-1, b'invalid argument: b747_ppo_rollout_population: params is NULL'),
    'b747_ppo_rollout_population/done_buf+fp32_state': (-1, b'invalid argument: b747_ppo_rollout_population: done_buf is NULL'),
    'b747_ppo_rollout_population/T+obs_dim_7': (-1, b'invalid argument: b747_ppo_rollout_population: T < 0'),
    'b747_ppo_rollout_population/n_negative+params': (-1, b'invalid argument: n < 0'),
    'b747_ppo_rollout_population/envs_per_policy_0': (-1, b'invalid argument: b747_ppo_rollout_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_ppo_rollout_population/envs_per_policy_100': (-1, b'invalid argument: b747_ppo_rollout_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_ppo_rollout_population/n_policies_0': (-1, b'invalid argument: b747_ppo_rollout_population: n_policies < 1'),
    'b747_ppo_rollout_population/n_below': (-1, b'invalid argument: b747_ppo_rollout_population: n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])'),
    'b747_ppo_rollout_population/n_above': (-1, b'invalid argument: b747_ppo_rollout_population: n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])'),
    'b747_ppo_rollout_population/stride_short': (-1, b'invalid argument: b747_ppo_rollout_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments start on a 16-byte boundary)'),
    'b747_ppo_rollout_population/stride_odd': (-1, b'invalid argument: b747_ppo_rollout_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments start on a 16-byte boundary)'),
    'b747_ppo_rollout_population/envs_per_policy+stride': (-1, b'invalid argument: b747_ppo_rollout_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_ppo_rollout_population/n_policies+n': (-1, b'invalid argument: b747_ppo_rollout_population: n_policies < 1'),
    'b747_ppo_rollout_population/n+stride': (-1, b'invalid argument: b747_ppo_rollout_population: n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])'),
    'b747_ppo_rollout_population/empty_batch': (-1, b'invalid argument: b747_ppo_rollout_population: n (an empty batch holds no group)'),
    'b747_ppo_rollout_population/empty_batch+params': (-1, b'invalid argument: b747_ppo_rollout_population: params is NULL'),
    'b747_ppo_rollout_population/empty_batch+envs_per_policy': (-1, b'invalid argument: b747_ppo_rollout_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_ppo_rollout_population/empty_batch+stride': (-1, b'invalid argument: b747_ppo_rollout_population: n (an empty batch holds no group)'),
    'b747_ppo_rollout_population/act_range+envs_per_policy': (-1, b'invalid argument: b747_ppo_rollout_population: act_lo > act_hi'),
    'b747_ppo_rollout_population/n_policies+obs_dim_7': (-1, b'invalid argument: b747_ppo_rollout_population: n_policies < 1'),
    'b747_ppo_rollout_population/recording+n': (-1, b'invalid argument: b747_ppo_rollout_population: sig (no per-DLL-step signal recording inside the rollout kernel)'),
    'b747_ppo_rollout_population/obs_dim_5_stride_of_3': (-1, b'invalid argument: b747_ppo_rollout_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments start on a 16-byte boundary)'),
    'b747_eval_episodes/y_base': (-1, b'invalid argument: y_base / eval_out is NULL'),
    'b747_eval_episodes/eval_out': (-1, b'invalid argument: y_base / eval_out is NULL'),
    'b747_eval_episodes/no_batch': (-1, b'invalid argument: env batch/config is NULL'),
    'b747_eval_episodes/consts': (-1, b'invalid argument: consts is NULL'),
    'b747_eval_episodes/steps': (-1, b'invalid argument: n_env_steps < 0'),
    'b747_eval_episodes/sig_row_negative': (-1, b'invalid argument: sig_row (a B747_SIG_* row)'),
    'b747_eval_episodes/sig_row_31': (-1, b'invalid argument: sig_row (a B747_SIG_* row)'),
    'b747_eval_episodes/act_range': (-1, b'invalid argument: act_lo > act_hi'),
    'b747_eval_episodes/fp32_state': (-1, b'invalid argument: b747_eval_episodes: x_f64 (the episode kernel keeps fp64 state only)'),
    'b747_eval_episodes/auto_reset': (-1, b'invalid argument: b747_eval_episodes: auto_reset must be 0 (an episode ends at its first done)'),
    'b747_eval_episodes/obs_dim_7': (-1, b'invalid argument: b747_eval_episodes: obs_dim (a policy runs with PID_LIKE 3 or SPEED_MODE 5 only; other observation types take params = NULL)'),
    'b747_eval_episodes/action': (-1, b'invalid argument: b747_eval_episodes: action is NULL (params = NULL holds b->action)'),
    'b747_eval_episodes/empty_batch': (0, b''),
    'b747_eval_episodes/consts+action': (-1, b'invalid argument: consts is NULL'),
    'b747_eval_episodes/y_base+fp32_state': (-1, b'invalid argument: y_base / eval_out is NULL'),
    'b747_eval_episodes/act_range+auto_reset': (-1, b'invalid argument: act_lo > act_hi'),
    'b747_eval_episodes/fp32_state+action': (-1, b'invalid argument: b747_eval_episodes: x_f64 (the episode kernel keeps fp64 state only)'),
    'b747_eval_population/y_base': (-1, b'invalid argument: b747_eval_population: y_base / eval_out is NULL'),
    'b747_eval_population/eval_out': (-1, b'invalid argument: b747_eval_population: y_base / eval_out is NULL'),
    'b747_eval_population/no_batch': (-1, b'invalid argument: env batch/config is NULL'),
    'b747_eval_population/consts': (-1, b'invalid argument: b747_eval_population: consts is NULL'),
    'b747_eval_population/steps': (-1, b'invalid argument: b747_eval_population: n_env_steps < 0'),
    'b747_eval_population/sig_row_negative': (-1, b'invalid argument: b747_eval_population: sig_row (a B747_SIG_* row)'),
    'b747_eval_population/sig_row_31': (-1, b'invalid argument: b747_eval_population: sig_row (a B747_SIG_* row)'),
    'b747_eval_population/act_range': (-1, b'invalid argument: b747_eval_population: act_lo > act_hi'),
    'b747_eval_population/fp32_state': (-1, b'invalid argument: b747_eval_population: x_f64 (the episode kernel keeps fp64 state only)'),
    'b747_eval_population/auto_reset': (-1, b'invalid argument: b747_eval_population: auto_reset must be 0 (an episode ends at its first done)'),
    'b747_eval_population/obs_dim_7': (-1, b'invalid argument: b747_eval_population: obs_dim (a policy runs with PID_LIKE 3 or SPEED_MODE 5 only; other observation types take params = NULL)'),
    'b747_eval_population/action': (-1, b'invalid argument: b747_eval_population: action is NULL (params = NULL holds b->action)'),
    'b747_eval_population/empty_batch': (0, b''),
    'b747_eval_population/consts+action': (-1, b'invalid argument: b747_eval_population: consts is NULL'),
    'b747_eval_population/y_base+fp32_state': (-1, b'invalid argument: b747_eval_population: y_base / eval_out is NULL'),
    'b747_eval_population/act_range+auto_reset': (-1, b'invalid argument: b747_eval_population: act_lo > act_hi'),
    'b747_eval_population/fp32_state+action': (-1, b'invalid argument: b747_eval_population: x_f64 (the episode kernel keeps fp64 state only)'),
    'b747_eval_population/envs_per_policy_0': (-1, b'invalid argument: b747_eval_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_eval_population/envs_per_policy_100': (-1, b'invalid argument: b747_eval_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_eval_population/n_policies_0': (-1, b'invalid argument: b747_eval_population: n_policies < 1 with params set'),
    'b747_eval_population/n_below': (-1, b'invalid argument: b747_eval_population: n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])'),
    'b747_eval_population/n_above': (-1, b'invalid argument: b747_eval_population: n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])'),
    'b747_eval_population/stride_short': (-1, b'invalid argument: b747_eval_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments start on a 16-byte boundary)'),
    'b747_eval_population/stride_odd': (-1, b'invalid argument: b747_eval_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments start on a 16-byte boundary)'),
    'b747_eval_population/envs_per_policy+stride': (-1, b'invalid argument: b747_eval_population: envs_per_policy (a positive multiple of 64: a wave flies one policy)'),
    'b747_eval_population/n_policies+n': (-1, b'invalid argument: b747_eval_population: n_policies < 1 with params set'),
    'b747_eval_population/n+stride': (-1, b'invalid argument: b747_eval_population: n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])'),
    'b747_eval_population/n_policies_without_params': (-1, b'invalid argument: b747_eval_population: n_policies must be 0 with params = NULL'),
    'b747_eval_population/action+n_policies': (-1, b'invalid argument: b747_eval_population: action is NULL (params = NULL holds b->action)'),
    'b747_eval_population/auto_reset+envs_per_policy': (-1, b'invalid argument: b747_eval_population: auto_reset must be 0 (an episode ends at its first done)'),
    'b747_eval_population/obs_dim_5_stride_of_3': (-1, b'invalid argument: b747_eval_population: policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments start on a 16-byte boundary)'),
}


def _call(L, name, over):
    """(return code, message) of the entry point with CALLS' arguments, `over` in place of some (a key the entry point
    does not take is left out: the case lists are shared).  An "env" argument stands for the three leading structures."""
    a = dict(CALLS[name])
    a.update({k: v for k, v in over.items() if k in a and k != "env"})
    keep, lead = [], []
    if "env" in a:
        e = dict(a.pop("env"), **over.get("env", {}))
        extra = {k: e.pop(k) for k in ("b", "cfg", "c", "auto_reset", "action") if k in e}
        keep = list(_env(**e))
        keep[1].auto_reset = extra.get("auto_reset", 0)
        if "action" in extra:
            keep[0].action = extra["action"]
        lead = [None if k in extra else ctypes.byref(s) for k, s in zip(("b", "cfg", "c"), keep)]
    if a.get("lr") == "host":
        a["lr"] = (ctypes.c_double * 3)(3e-4, 3e-4, 3e-4)
    code = int(getattr(L, name)(*lead, *a.values()))
    return code, bytes(L.b747_last_error()) if code != 0 else b""


def _ids():
    return [(name, case, over) for name, cases in CASES.items() for case, over in cases]


def test_the_table_has_every_case_once():
    from b747_rl_ctrl_amd import _lib
    assert int(_lib.lib().b747_policy_num_params(3)) == NUM3
    ids = ["%s/%s" % (n, c) for n, c, _ in _ids()]
    assert len(ids) == len(set(ids)) and sorted(ids) == sorted(EXPECTED)
    for name, cases in CASES.items():
        assert len(_lib.SIGNATURES[name][0]) == len(CALLS[name]) + (2 if "env" in CALLS[name] else 0), name
        assert sum("+" in c for c, _ in cases) >= 2 or name == "b747_ppo_rollout", name   # (order cases)


@pytest.mark.parametrize("name,case,over", _ids(), ids=["%s/%s" % (n, c) for n, c, _ in _ids()])
def test_the_return_code_and_the_message(name, case, over):
    from b747_rl_ctrl_amd import _lib
    got = _call(_lib.lib(), name, over)
    assert got == EXPECTED["%s/%s" % (name, case)], got


if __name__ == "__main__":
    from b747_rl_ctrl_amd import _lib
    print("EXPECTED = {")
    for name, case, over in _ids():
        print("    %r: %r," % ("%s/%s" % (name, case), _call(_lib.lib(), name, over)))
    print("}")
