// b747_kernels.hip -- MI355X (gfx950) kernels + C ABI of libb747.so.
//
// One lane = one environment = one copy of the reference DLL's static model state
// (core/model_simple_win64.dll; the reference loads a file copy of the DLL per env,
// core/model.py:99-110).  State is structure-of-arrays in HBM ([field][N]) so that each
// wave64 load/store of a field is one contiguous 256 B (fp32) / 512 B (fp64) transaction.
// The 241 lookup-table doubles (CYa, CXa, dCm/ddeltaz, mz, K_alpha) are staged into LDS once
// per workgroup; per-lane table gathers then hit LDS, not L1/L2.
//
// Roofline: with n_steps == 1 a step moves the whole compact state through HBM
// (algorithmic bytes in DESIGN.md); with n_steps > 1 state stays in VGPRs and the kernel is
// fp64-VALU bound (4 output passes x ~11 transcendentals per step).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../include/b747.h"
#include "b747_dynamics.h"
#include "b747_env.h"
#include "b747_lanes.h"
#include "b747_policy.h"
#include "b747_eval_args.h"
#define B747_ROLLOUT_LANES_NO_KERNELS   // k_rollout_lanes lives in b747_rollout_lanes_{fast,faithful}.hip
#include "b747_rollout_lanes.h"
#define B747_PPO_UPDATE_NO_KERNELS   // the update kernels live in b747_ppo_update.hip; this unit calls their launchers
#include "b747_ppo_update.h"
#include "b747_a2c_update.h"
#include "b747_a2c_population.h"
#include "b747_ppo_gae.h"
#include "b747_ppo_order.h"
#include "b747_ppo_track.h"
#include "b747_ppo_exploit.h"

using namespace b747;

#define B747_API __attribute__((visibility("default")))

namespace {

thread_local char g_err[256] = "";

int32_t fail(hipError_t e, const char *where)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return -(int32_t)e;
}

// where: the entry point's name in front of the message, or nullptr for the older entry points, whose messages carry none
int32_t bad_arg(const char *where, const char *what)
{
    if (where) snprintf(g_err, sizeof(g_err), "invalid argument: %s: %s", where, what);
    else snprintf(g_err, sizeof(g_err), "invalid argument: %s", what);
    return -(int32_t)hipErrorInvalidValue;
}
int32_t bad_arg(const char *what) { return bad_arg(nullptr, what); }

// the tail of every entry point that launches: 0, or the launch's error under the entry point's name
int32_t launched(const char *where, hipError_t e = hipGetLastError()) { return e == hipSuccess ? 0 : fail(e, where); }

// a launcher was handed a plan whose kernel its translation unit does not have: a bug in the dispatch, never a
// fallback to another kernel
int32_t bad_plan(const char *where)
{
    snprintf(g_err, sizeof(g_err), "%s: internal error: the launch plan names a kernel its launcher does not have", where);
    return -(int32_t)hipErrorInvalidDeviceFunction;
}

int32_t check_env(const b747_env_batch *b, const b747_env_config *cfg)
{
    if (!b || !cfg) return bad_arg("env batch/config is NULL");
    if (b->n < 0) return bad_arg("n < 0");
    if (b->n == 0) return 0;
    if (!b->X || !b->disc || !b->k || !b->mem || !b->deltaz || !b->vartheta || !b->h_zh || !b->upid ||
        !b->tp || !b->flags || !b->aero_err || !b->ref || !b->ref_kind || !b->episode || !b->ep_return ||
        !b->ep_len || !b->obs || !b->reward || !b->done)
        return bad_arg("env batch pointer is NULL");
    if (cfg->obs_type < 0 || cfg->obs_type > 4) return bad_arg("obs_type");
    if (b->obs_dim != obs_dim_of(cfg->obs_type)) return bad_arg("obs_dim does not match obs_type");
    if (cfg->reward_type < 0 || cfg->reward_type > 4) return bad_arg("reward_type");
    if (cfg->n_sub < 1) return bad_arg("n_sub < 1 (sample_time < dt)");
    if (cfg->ctrl_mode < -1 || cfg->ctrl_mode > 3) return bad_arg("ctrl_mode");
    if (cfg->reset_ref_mode < -1 || cfg->reset_ref_mode > 2) return bad_arg("reset_ref_mode");
    return 1;
}

Consts consts_of(const b747_consts *c)
{
    return make_consts(c->Iz, c->P, c->S, c->c_, c->g, c->m0, c->PID_CS, c->PID_SS);
}

// b747_set_specialization's setting (plan_env / plan_model, b747_dispatch.h): the specialised kernels are on by default
static int32_t g_spec = 1;

int32_t check_batch(const b747_model_batch *b, bool need_params)
{
    if (!b) return bad_arg("batch is NULL");
    if (b->n < 0) return bad_arg("n < 0");
    if (b->n == 0) return 0;
    if (!b->X || !b->disc || !b->k || !b->mem) return bad_arg("state pointer is NULL");
    if (need_params && (!b->deltaz || !b->vartheta || !b->h_zh || !b->flags || !b->aero_err))
        return bad_arg("parameter pointer is NULL");
    return 1;
}

// Never launched.  The hand-written dispatch this unit had before the launch plans instantiated these two as a
// by-product (its FAITHFUL spelling of the K1 launch, behind a condition that was always false); they stay so that the
// library's kernel set is what it was (profiles/refactor_dispatch/isa_diff.txt).  Deleting them changes nothing else.
template __global__ void k_env_steps<double, false, 1, true>(b747_env_batch, b747_env_config, Consts, const float *,
                                                            int32_t, float *, float *, uint8_t *);
template __global__ void k_env_steps<float, false, 1, true>(b747_env_batch, b747_env_config, Consts, const float *,
                                                           int32_t, float *, float *, uint8_t *);

// The validators below are shared by the entry points of one family: 0, or bad_arg's code with the message under
// `where` (nullptr: no name).  The order of the checks is part of the ABI: it decides the message of a doubly-wrong call.

// "<name> is NULL" for the first null pointer of the list
struct NamedPtr {
    const void *p;
    const char *name;
};
int32_t check_not_null(const char *where, std::initializer_list<NamedPtr> ptrs)
{
    char what[64];
    for (const NamedPtr &a : ptrs) {
        if (a.p) continue;
        snprintf(what, sizeof(what), "%s is NULL", a.name);
        return bad_arg(where, what);
    }
    return 0;
}

bool policy_stride_ok(int64_t policy_stride, int32_t od)
{
    return policy_stride >= policy_total_params(od) && policy_stride % 4 == 0;
}

// --- the update family (b747_ppo_grad, _epoch, _epoch_population, _epoch_batched), in three parts around the entry
// points' own checks: the policy; the members; the rows (epoch false: b747_ppo_grad's one minibatch `idx` of n_rows)
int32_t check_upd_policy(const char *where, const float *theta, int32_t obs_dim)
{
    if (!theta) return bad_arg(where, "theta is NULL");
    if (!policy_obs_dim_ok(obs_dim)) return bad_arg(where, "obs_dim (3, 5, 7, 8 or 10)");
    return 0;
}
int32_t check_upd_members(const char *where, int32_t n_policies, int64_t policy_stride, int32_t obs_dim)
{
    if (n_policies < 1) return bad_arg(where, "n_policies < 1");
    if (!policy_stride_ok(policy_stride, obs_dim))
        return bad_arg(where, "policy_stride (at least b747_policy_num_params floats and a multiple of 4)");
    return 0;
}
int32_t check_upd_rows(const char *where, const UpdData &d, const int64_t *idx, bool epoch, int64_t n_rows,
                       int64_t batch_size, const void *workspace)
{
    if (int32_t e = check_not_null(where, {{d.obs, "obs"}, {d.act, "act"}, {d.old_logp, "old_logp"}, {d.adv, "adv"},
                                           {d.ret, "ret"}, {idx, epoch ? "perm" : "idx"}}))
        return e;
    if (!epoch) {
        if (n_rows < 2) return bad_arg(where, "batch < 2 (the advantages' standard deviation needs two rows)");
    } else {
        if (n_rows < 2) return bad_arg(where, "n_rows < 2 (the advantages' standard deviation needs two rows)");
        if (batch_size < 2) return bad_arg(where, "batch_size < 2 (the advantages' standard deviation needs two rows)");
        if (n_rows % batch_size == 1)
            return bad_arg(where, "n_rows % batch_size == 1 (the last minibatch would be one row: no standard deviation)");
    }
    return check_not_null(where, {{workspace, "workspace"}});
}

// --- the A2C family (b747_a2c_grad, b747_ppo_rmsprop, b747_a2c_update), in two parts: the rows (idx may be NULL), the
// optimiser's scalars (alpha: RMSprop's only)
int32_t check_a2c_rows(const char *where, const float *theta, int32_t obs_dim, const UpdData &d, int64_t batch,
                       int32_t normalize_advantage, const void *workspace, const float *grad, const float *stats)
{
    if (int32_t e = check_upd_policy(where, theta, obs_dim)) return e;
    if (int32_t e = check_not_null(where, {{d.obs, "obs"}, {d.act, "act"}, {d.adv, "adv"}, {d.ret, "ret"}})) return e;
    if (batch < 1) return bad_arg(where, "batch < 1");
    if (normalize_advantage && batch < 2)
        return bad_arg(where, "batch < 2 with normalize_advantage (the advantages' standard deviation needs two rows)");
    return check_not_null(where, {{workspace, "workspace"}, {grad, "grad"}, {stats, "stats"}});
}
int32_t check_opt_scalars(const char *where, int64_t n_params, double max_grad_norm, double lr, double eps,
                          bool rmsprop, double alpha)
{
    if (n_params < 1) return bad_arg(where, "n_params < 1");
    if (!(isfinite(max_grad_norm) && max_grad_norm > 0.0)) return bad_arg(where, "max_grad_norm (not finite and above 0)");
    if (!(isfinite(lr) && lr > 0.0)) return bad_arg(where, "lr (not finite and above 0)");
    if (!(isfinite(eps) && eps > 0.0)) return bad_arg(where, "eps (not finite and above 0)");
    if (rmsprop && !(alpha >= 0.0 && alpha < 1.0)) return bad_arg(where, "alpha (outside [0, 1))");
    return 0;
}

// --- the population tiling (b747_eval_population, b747_ppo_rollout_population), in two parts: the groups, then -- once
// the batch is known not to be empty -- the batch's place in them and the parameter sets' distance
int32_t check_pop_groups(const char *where, int32_t envs_per_policy, int32_t n_policies, const char *few_policies)
{
    if (envs_per_policy < 64 || envs_per_policy % 64 != 0)
        return bad_arg(where, "envs_per_policy (a positive multiple of 64: a wave flies one policy)");
    if (n_policies < 1) return bad_arg(where, few_policies);
    return 0;
}
int32_t check_pop_tiling(const char *where, const b747_env_batch &b, int32_t n_policies, int32_t envs_per_policy,
                         int64_t policy_stride)
{
    if (b.n <= (int64_t)(n_policies - 1) * envs_per_policy || b.n > (int64_t)n_policies * envs_per_policy)
        return bad_arg(where, "n (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])");
    if (!policy_stride_ok(policy_stride, b.obs_dim))
        return bad_arg(where, "policy_stride (at least b747_policy_num_params floats and a multiple of 4: the fragments "
                              "start on a 16-byte boundary)");
    return 0;
}

// --- the rollout buffers (b747_ppo_rollout_lanes, b747_ppo_rollout_population)
int32_t check_rollout_args(const char *where, const b747_consts *c, const RolloutLanesArgs &ra)
{
    if (int32_t e = check_not_null(where, {{c, "consts"}, {ra.params, "params"}, {ra.obs_buf, "obs_buf"},
                                           {ra.act_buf, "act_buf"}, {ra.logp_buf, "logp_buf"}, {ra.val_buf, "val_buf"},
                                           {ra.rew_buf, "rew_buf"}, {ra.done_buf, "done_buf"}}))
        return e;
    if (ra.T < 0) return bad_arg(where, "T < 0");
    if (!(ra.act_lo <= ra.act_hi)) return bad_arg(where, "act_lo > act_hi");
    return 0;
}

// --- the step-response arguments (b747_eval_episodes, b747_eval_population).  b747_eval_episodes names itself in the
// messages about the batch only: `where` is nullptr there, `name` the entry point's in both
int32_t check_eval_args(const char *where, const char *name, const b747_env_batch &b, const b747_env_config &cfg,
                        const b747_consts *c, const EvalArgs &ea)
{
    if (!c) return bad_arg(where, "consts is NULL");
    if (!ea.y_base || !ea.out) return bad_arg(where, "y_base / eval_out is NULL");
    if (ea.n_env_steps < 0) return bad_arg(where, "n_env_steps < 0");
    if (ea.sig_row < 0 || ea.sig_row >= B747_NSIG) return bad_arg(where, "sig_row (a B747_SIG_* row)");
    if (!(ea.act_lo <= ea.act_hi)) return bad_arg(where, "act_lo > act_hi");
    if (!b.x_f64) return bad_arg(name, "x_f64 (the episode kernel keeps fp64 state only)");
    if (cfg.auto_reset != 0) return bad_arg(name, "auto_reset must be 0 (an episode ends at its first done)");
    if (ea.params && b.obs_dim != 3 && b.obs_dim != 5)
        return bad_arg(name, "obs_dim (a policy runs with PID_LIKE 3 or SPEED_MODE 5 only; other observation types take "
                             "params = NULL)");
    if (!ea.params && !b.action) return bad_arg(name, "action is NULL (params = NULL holds b->action)");
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------ C ABI ----
extern "C" {

B747_API int32_t b747_abi_version(void) { return B747_ABI_VERSION; }

B747_API int64_t b747_struct_size(int32_t which)
{
    switch (which) {
    case B747_STRUCT_CONSTS: return (int64_t)sizeof(b747_consts);
    case B747_STRUCT_MODEL_BATCH: return (int64_t)sizeof(b747_model_batch);
    case B747_STRUCT_ENV_CONFIG: return (int64_t)sizeof(b747_env_config);
    case B747_STRUCT_ENV_BATCH: return (int64_t)sizeof(b747_env_batch);
    default: return -1;
    }
}

B747_API const char *b747_last_error(void) { return g_err; }

B747_API int32_t b747_policy_num_params(int32_t obs_dim)
{
    if (obs_dim < 1 || obs_dim > 10) return bad_arg("obs_dim");
    return policy_total_params(obs_dim);
}

B747_API int32_t b747_policy_pack(float *params, int32_t obs_dim, void *stream)
{
    if (!params) return bad_arg("params is NULL");
    if (obs_dim < 1 || obs_dim > 10) return bad_arg("obs_dim");
    hipLaunchKernelGGL(k_policy_pack, dim3((policy_pack_threads(obs_dim) + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       params, (int)obs_dim);
    return launched("b747_policy_pack");
}

B747_API int32_t b747_policy_act(const float *params, int32_t obs_dim, int64_t n, const float *obs, const float *noise,
                                 uint64_t seed, const uint64_t *step_base, uint32_t step, int64_t env_offset,
                                 float *obs_out, float *act_out, float *logp_out, float *value_out, float *env_action,
                                 float act_lo, float act_hi, void *stream)
{
    if (n < 0) return bad_arg("n < 0");
    if (n == 0) return 0;
    if (!params || !obs || !act_out || !logp_out || !value_out || !env_action) return bad_arg("NULL buffer");
    if (!(act_lo <= act_hi)) return bad_arg("act_lo > act_hi");
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(grid_for(n)), blk(kBlock);
    const bool known = with_obs_dim(obs_dim, false, [&](auto OD) {
        hipLaunchKernelGGL(k_policy_act<OD()>, g, blk, 0, s, params, n, obs, noise, seed, step_base, step, env_offset,
                           obs_out, act_out, logp_out, value_out, env_action, act_lo, act_hi);
        return true;
    });
    if (!known) return bad_arg("obs_dim (PID_LIKE 3, SPEED_MODE 5, MODEL_STATE 7, PID_AERO 8, PID_SPEED_AERO 10)");
    return launched("b747_policy_act");
}

B747_API int32_t b747_ppo_rollout(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                  const float *params, uint64_t seed, uint64_t *step_base, int32_t T, float *obs_buf,
                                  float *act_buf, float *logp_buf, float *val_buf, float *rew_buf, uint8_t *done_buf,
                                  float act_lo, float act_hi, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r <= 0) return r;
    if (!c || !params || !obs_buf || !act_buf || !logp_buf || !val_buf || !rew_buf || !done_buf)
        return bad_arg("NULL buffer");
    if (T < 0) return bad_arg("T < 0");
    if (!(act_lo <= act_hi)) return bad_arg("act_lo > act_hi");
    if (!ppo_rollout_covers(*b, *cfg, is_default(*c)))
        return bad_arg("b747_ppo_rollout: the fused kernel covers the training configuration only (default "
                       "constants, PID_LIKE/CLASSIC/MANUAL-DIRECT/CONST/AERO, fp64 state, FAST, n % 64 == 0); "
                       "use b747_policy_act + b747_env_step");
    if (T == 0) return 0;
    launch_ppo_rollout_fast(*b, *cfg, params, seed, step_base, T, obs_buf, act_buf, logp_buf, val_buf, rew_buf, done_buf,
                            act_lo, act_hi, (hipStream_t)stream);
    // the value head of every observation the rollout stored (V(obs_t), the rollout's parameters): one batched
    // launch after the rollout instead of inside its latency-bound step loop; it also advances *step_base by T
    const int64_t rows = (int64_t)T * b->n;
    hipLaunchKernelGGL(k_policy_value<3>, dim3((unsigned)policy_value_blocks(rows)), dim3(256), 0, (hipStream_t)stream,
                       params, rows, obs_buf, val_buf, step_base, (uint32_t)T);
    return launched("b747_ppo_rollout");
}

B747_API int32_t b747_ppo_rollout_lanes(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                        const float *params, uint64_t seed, uint64_t *step_base, int32_t T,
                                        float *obs_buf, float *act_buf, float *logp_buf, float *val_buf, float *rew_buf,
                                        uint8_t *done_buf, float act_lo, float act_hi, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r < 0) return r;
    const RolloutLanesArgs ra{params, seed, step_base, T, act_lo, act_hi, obs_buf, act_buf, logp_buf, val_buf, rew_buf,
                              done_buf};
    if (int32_t e = check_rollout_args("b747_ppo_rollout_lanes", c, ra)) return e;
    if (r == 0) return 0;   // an empty batch
    if (const char *why = ppo_rollout_lanes_refusal(*b)) return bad_arg(why);
    if (T == 0) return 0;
    const Consts C = consts_of(c);   // run-time constants, as the evaluation kernel
    // (the launcher's second launch advances *step_base by T: ordered after the rollout kernel's last read of it;
    //  where the value head is deferred, b747_ppo_rollout's value pass does both)
    const bool defer = kLanesDeferValue3 && b->obs_dim == 3;
    uint64_t *advance = defer ? nullptr : step_base;
    if (b->variant != B747_VARIANT_FAITHFUL)
        launch_rollout_lanes_fast(*b, *cfg, C, ra, b->obs_dim, advance, (hipStream_t)stream);
    else launch_rollout_lanes_faithful(*b, *cfg, C, ra, b->obs_dim, advance, (hipStream_t)stream);
    if (defer) {
        const int64_t rows = (int64_t)T * b->n;
        hipLaunchKernelGGL(k_policy_value<3>, dim3((unsigned)policy_value_blocks(rows)), dim3(256), 0,
                           (hipStream_t)stream, params, rows, obs_buf, val_buf, step_base, (uint32_t)T);
    }
    return launched("b747_ppo_rollout_lanes");
}

B747_API int32_t b747_eval_episodes(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                    const float *params, int32_t n_env_steps, int32_t sig_row, double scale,
                                    const double *y_base, double error_band, float act_lo, float act_hi,
                                    double *eval_out, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r <= 0) return r;
    const EvalArgs ea{params, n_env_steps, sig_row, scale, y_base, error_band, act_lo, act_hi, eval_out};
    if (int32_t e = check_eval_args(nullptr, "b747_eval_episodes", *b, *cfg, c, ea)) return e;
    if (n_env_steps == 0) return 0;
    const Consts C = consts_of(c);   // run-time constants: no instantiation of this kernel needs the DLL's defaults
    const int od = params ? b->obs_dim : 0;
    if (b->variant != B747_VARIANT_FAITHFUL) launch_eval_episodes_fast(*b, *cfg, C, ea, od, (hipStream_t)stream);
    else launch_eval_episodes_faithful(*b, *cfg, C, ea, od, (hipStream_t)stream);
    return launched("b747_eval_episodes");
}

B747_API int32_t b747_policy_pack_batch(float *params, int32_t obs_dim, int32_t n_policies, int64_t policy_stride,
                                        void *stream)
{
    if (!params) return bad_arg("b747_policy_pack_batch: params is NULL");
    if (obs_dim < 1 || obs_dim > 10) return bad_arg("b747_policy_pack_batch: obs_dim");
    if (n_policies < 0 || n_policies > 65535) return bad_arg("b747_policy_pack_batch: n_policies (0 .. 65535)");
    if (!policy_stride_ok(policy_stride, obs_dim))
        return bad_arg("b747_policy_pack_batch: policy_stride (at least b747_policy_num_params floats, a multiple of 4)");
    if (n_policies == 0) return 0;
    hipLaunchKernelGGL(k_policy_pack_batch, dim3((policy_pack_threads(obs_dim) + 255) / 256, (unsigned)n_policies),
                       dim3(256), 0, (hipStream_t)stream, params, (int)obs_dim, policy_stride);
    return launched("b747_policy_pack_batch");
}

B747_API int32_t b747_eval_population(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                      const float *params, int32_t n_policies, int64_t policy_stride,
                                      int32_t envs_per_policy, const double *pid_ss, const double *pid_cs,
                                      int32_t n_env_steps, int32_t sig_row, double scale, const double *y_base,
                                      double error_band, float act_lo, float act_hi, double *eval_out, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r <= 0) return r;
    const char *const W = "b747_eval_population";
    const EvalArgs ea{params, n_env_steps, sig_row, scale, y_base, error_band, act_lo, act_hi, eval_out};
    if (int32_t e = check_eval_args(W, W, *b, *cfg, c, ea)) return e;
    if (params) {
        if (int32_t e = check_pop_groups(W, envs_per_policy, n_policies, "n_policies < 1 with params set")) return e;
        if (int32_t e = check_pop_tiling(W, *b, n_policies, envs_per_policy, policy_stride)) return e;
    } else if (n_policies != 0) {
        return bad_arg(W, "n_policies must be 0 with params = NULL");
    }
    if (n_env_steps == 0) return 0;
    const PopArgs pa{policy_stride, params ? envs_per_policy / 64 : 1, pid_ss, pid_cs};
    const Consts C = consts_of(c);
    const int od = params ? b->obs_dim : 0;
    if (b->variant != B747_VARIANT_FAITHFUL) launch_eval_population_fast(*b, *cfg, C, ea, pa, od, (hipStream_t)stream);
    else launch_eval_population_faithful(*b, *cfg, C, ea, pa, od, (hipStream_t)stream);
    return launched("b747_eval_population");
}

B747_API int32_t b747_ppo_rollout_population(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                             const float *params, int32_t n_policies, int64_t policy_stride,
                                             int32_t envs_per_policy, const double *rew_pop, uint64_t seed,
                                             uint64_t *step_base, int32_t T, float *obs_buf, float *act_buf,
                                             float *logp_buf, float *val_buf, float *rew_buf, uint8_t *done_buf,
                                             float *last_val, float act_lo, float act_hi, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r < 0) return r;
    const char *const W = "b747_ppo_rollout_population";
    const RolloutLanesArgs ra{params, seed, step_base, T, act_lo, act_hi, obs_buf, act_buf, logp_buf, val_buf, rew_buf,
                              done_buf};
    if (int32_t e = check_rollout_args(W, c, ra)) return e;
    if (int32_t e = check_pop_groups(W, envs_per_policy, n_policies, "n_policies < 1")) return e;
    if (r == 0) return bad_arg(W, "n (an empty batch holds no group)");
    if (b->obs_dim != 3 && b->obs_dim != 5)
        return bad_arg(W, "obs_dim (the one-wave rollout kernel runs a policy with PID_LIKE 3 or SPEED_MODE 5 only)");
    if (!b->x_f64) return bad_arg(W, "x_f64 (the one-wave rollout kernel keeps fp64 state only)");
    if (b->sig) return bad_arg(W, "sig (no per-DLL-step signal recording inside the rollout kernel)");
    if (int32_t e = check_pop_tiling(W, *b, n_policies, envs_per_policy, policy_stride)) return e;
    if (T == 0) return 0;
    const RolloutPopArgs pa{policy_stride, envs_per_policy / 64, rew_pop, last_val};
    const Consts C = consts_of(c);
    // (the launcher's second launch advances *step_base by T: ordered after the rollout kernel's last read of it)
    if (b->variant != B747_VARIANT_FAITHFUL)
        launch_rollout_population_fast(*b, *cfg, C, ra, pa, b->obs_dim, step_base, (hipStream_t)stream);
    else launch_rollout_population_faithful(*b, *cfg, C, ra, pa, b->obs_dim, step_base, (hipStream_t)stream);
    return launched("b747_ppo_rollout_population");
}

B747_API int64_t b747_ppo_update_workspace(int32_t obs_dim)
{
    if (!policy_obs_dim_ok(obs_dim)) return bad_arg("obs_dim (3, 5, 7, 8 or 10)");
    return upd_ws_bytes(obs_dim);
}

B747_API int32_t b747_ppo_grad(const float *theta, int32_t obs_dim, const float *obs, const float *act,
                               const float *old_logp, const float *adv, const float *ret, const int64_t *idx,
                               int64_t batch, double clip_range, double ent_coef, double vf_coef, void *workspace,
                               float *grad, float *stats, void *stream)
{
    const UpdData d{obs, act, old_logp, adv, ret};
    if (int32_t e = check_upd_policy(nullptr, theta, obs_dim)) return e;
    if (int32_t e = check_upd_rows(nullptr, d, idx, false, batch, 0, workspace)) return e;
    if (int32_t e = check_not_null(nullptr, {{grad, "grad"}, {stats, "stats"}})) return e;
    return launched("b747_ppo_grad", launch_ppo_grad(theta, obs_dim, d, idx, batch, {clip_range, ent_coef, vf_coef},
                                                     workspace, grad, stats, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_adam(float *theta, float *m, float *v, int64_t *t, const float *grad, int64_t n_params,
                               double grad_scale, double max_grad_norm, double lr, double beta1, double beta2,
                               double eps, void *stream)
{
    if (int32_t e = check_not_null(nullptr, {{theta, "theta"}, {m, "m"}, {v, "v"}, {t, "t"}, {grad, "grad"}})) return e;
    if (n_params < 1) return bad_arg("n_params < 1");
    return launched("b747_ppo_adam", launch_ppo_adam({theta, m, v, t}, grad, n_params, grad_scale,
                                                     {max_grad_norm, beta1, beta2, eps}, lr, (hipStream_t)stream));
}

B747_API int32_t b747_a2c_grad(const float *theta, int32_t obs_dim, const float *obs, const float *act, const float *adv,
                               const float *ret, const int64_t *idx, int64_t batch, int32_t normalize_advantage,
                               double ent_coef, double vf_coef, void *workspace, float *grad, float *stats, void *stream)
{
    const char *const W = "b747_a2c_grad";
    const UpdData d{obs, act, nullptr, adv, ret};
    if (int32_t e = check_a2c_rows(W, theta, obs_dim, d, batch, normalize_advantage, workspace, grad, stats)) return e;
    return launched(W, launch_a2c_grad(theta, obs_dim, d, idx, batch, normalize_advantage != 0, ent_coef, vf_coef,
                                       workspace, grad, stats, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_rmsprop(float *theta, float *sq, int64_t *t, const float *grad, int64_t n_params,
                                  double grad_scale, double max_grad_norm, double lr, double alpha, double eps,
                                  int32_t tf_like, void *stream)
{
    const char *const W = "b747_ppo_rmsprop";
    if (int32_t e = check_not_null(W, {{theta, "theta"}, {sq, "sq"}, {t, "t"}, {grad, "grad"}})) return e;
    if (int32_t e = check_opt_scalars(W, n_params, max_grad_norm, lr, eps, true, alpha)) return e;
    return launched(W, launch_ppo_rmsprop(theta, sq, t, grad, n_params, grad_scale,
                                          {max_grad_norm, alpha, eps, tf_like != 0}, lr, (hipStream_t)stream));
}

B747_API int32_t b747_a2c_update(float *theta, int32_t obs_dim, const float *obs, const float *act, const float *adv,
                                 const float *ret, const int64_t *idx, int64_t batch, int32_t normalize_advantage,
                                 double ent_coef, double vf_coef, void *workspace, float *grad, float *stats,
                                 int32_t optimizer, float *state0, float *state1, int64_t *t, double max_grad_norm,
                                 double lr, double alpha, double eps, void *stream)
{
    const char *const W = "b747_a2c_update";
    const UpdData d{obs, act, nullptr, adv, ret};
    if (int32_t e = check_a2c_rows(W, theta, obs_dim, d, batch, normalize_advantage, workspace, grad, stats)) return e;
    if (optimizer != B747_OPT_ADAM && optimizer != B747_OPT_RMSPROP && optimizer != B747_OPT_RMSPROP_TF)
        return bad_arg(W, "optimizer (B747_OPT_ADAM, B747_OPT_RMSPROP or B747_OPT_RMSPROP_TF)");
    const bool adam = optimizer == B747_OPT_ADAM;
    if (int32_t e = check_not_null(W, {{state0, "state0"}, {adam ? state1 : state0, "state1"}, {t, "t"}})) return e;
    const int64_t n_params = PolicyLayout::of(obs_dim).total;
    if (int32_t e = check_opt_scalars(W, n_params, max_grad_norm, lr, eps, !adam, alpha)) return e;
    const hipStream_t s = (hipStream_t)stream;
    if (int32_t e = launched(W, launch_a2c_grad(theta, obs_dim, d, idx, batch, normalize_advantage != 0, ent_coef,
                                                vf_coef, workspace, grad, stats, s)))
        return e;
    if (adam)
        return launched(W, launch_ppo_adam({theta, state0, state1, t}, grad, n_params, 1.0,
                                           {max_grad_norm, 0.9, 0.999, eps}, lr, s));
    return launched(W, launch_ppo_rmsprop(theta, state0, t, grad, n_params, 1.0,
                                          {max_grad_norm, alpha, eps, optimizer == B747_OPT_RMSPROP_TF}, lr, s));
}

B747_API int32_t b747_a2c_update_population(float *theta, int32_t n_policies, int64_t policy_stride, int32_t obs_dim,
                                            const float *obs, const float *act, const float *adv, const float *ret,
                                            const int64_t *rows, int64_t rows_stride, int64_t batch,
                                            int32_t normalize_advantage, const double *hyper_dev, void *workspace,
                                            int64_t workspace_bytes, float *state0, float *state1, int64_t *t,
                                            double rms_alpha, double rms_eps, double adam_beta1, double adam_beta2,
                                            double adam_eps, float *stats, void *stream)
{
    const char *const W = "b747_a2c_update_population";
    const UpdData d{obs, act, nullptr, adv, ret};
    if (int32_t e = check_upd_policy(W, theta, obs_dim)) return e;
    if (int32_t e = check_upd_members(W, n_policies, policy_stride, obs_dim)) return e;
    if (int32_t e = check_not_null(W, {{obs, "obs"}, {act, "act"}, {adv, "adv"}, {ret, "ret"}, {rows, "rows"}})) return e;
    if (batch < 1) return bad_arg(W, "batch < 1");
    if (normalize_advantage && batch < 2)
        return bad_arg(W, "batch < 2 with normalize_advantage (the advantages' standard deviation needs two rows)");
    if (rows_stride < batch) return bad_arg(W, "rows_stride < batch (a member's row of the index table holds its batch)");
    if (!hyper_dev)
        return bad_arg(W, "hyper_dev is NULL (a device table, one row of B747_PPO_HYPER_COLS doubles per member)");
    if (int32_t e = check_not_null(W, {{workspace, "workspace"}})) return e;
    if (workspace_bytes < upd_pop_ws_bytes(obs_dim, batch))
        return bad_arg(W, "workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch))");
    if (int32_t e = check_not_null(W, {{state0, "state0"}, {state1, "state1"}, {t, "t"}})) return e;
    if (!(rms_alpha >= 0.0 && rms_alpha < 1.0)) return bad_arg(W, "rms_alpha (outside [0, 1))");
    if (!(isfinite(rms_eps) && rms_eps > 0.0)) return bad_arg(W, "rms_eps (not finite and above 0)");
    if (!(adam_beta1 >= 0.0 && adam_beta1 < 1.0)) return bad_arg(W, "adam_beta1 (outside [0, 1))");
    if (!(adam_beta2 >= 0.0 && adam_beta2 < 1.0)) return bad_arg(W, "adam_beta2 (outside [0, 1))");
    if (!(isfinite(adam_eps) && adam_eps > 0.0)) return bad_arg(W, "adam_eps (not finite and above 0)");
    if (!stats) return bad_arg(W, "stats is NULL");
    return launched(W, launch_a2c_update_population({theta, state0, state1, t}, n_policies, policy_stride, obs_dim, d,
                                                    rows, rows_stride, batch, normalize_advantage != 0, hyper_dev,
                                                    workspace, workspace_bytes,
                                                    {rms_alpha, rms_eps, adam_beta1, adam_beta2, adam_eps}, stats,
                                                    (hipStream_t)stream));
}

B747_API int32_t b747_ppo_gae(const float *rew, const float *val, const uint8_t *done, const float *last_value,
                              int32_t T, int64_t N, double gamma, double gae_lambda, float *adv, float *ret,
                              void *stream)
{
    if (!rew) return bad_arg("rew is NULL");
    if (!val) return bad_arg("val is NULL");
    if (!done) return bad_arg("done is NULL");
    if (!last_value) return bad_arg("last_value is NULL");
    if (!adv) return bad_arg("adv is NULL");
    if (!ret) return bad_arg("ret is NULL");
    if (T < 0) return bad_arg("T < 0");
    if (N < 0) return bad_arg("N < 0");
    if (N > (int64_t)kGaeBlock * INT32_MAX) return bad_arg("N (more envs than one grid holds)");
    if (T == 0 || N == 0) return 0;
    return launched("b747_ppo_gae",
                    launch_ppo_gae(rew, val, done, last_value, T, N, gamma, gae_lambda, adv, ret, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_gae_population(const float *rew, const float *val, const uint8_t *done,
                                         const float *last_value, int32_t T, int64_t N, int32_t n_policies,
                                         int32_t envs_per_policy, const double *hyper_dev, float *adv, float *ret,
                                         void *stream)
{
    const char *const W = "b747_ppo_gae_population";
    if (int32_t e = check_not_null(W, {{rew, "rew"}, {val, "val"}, {done, "done"}, {last_value, "last_value"},
                                       {hyper_dev, "hyper_dev"}, {adv, "adv"}, {ret, "ret"}}))
        return e;
    if (T < 0) return bad_arg(W, "T < 0");
    if (N < 0) return bad_arg(W, "N < 0");
    if (int32_t e = check_pop_groups(W, envs_per_policy, n_policies, "n_policies < 1")) return e;
    if (N == 0) return 0;
    // (the upper bound keeps every workgroup's member inside the table)
    if (N <= (int64_t)(n_policies - 1) * envs_per_policy || N > (int64_t)n_policies * envs_per_policy)
        return bad_arg(W, "N (outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy])");
    if (N > (int64_t)kGaeBlock * INT32_MAX) return bad_arg(W, "N (more envs than one grid holds)");
    if (T == 0) return 0;
    return launched(W, launch_ppo_gae_population(rew, val, done, last_value, T, N, envs_per_policy, hyper_dev, adv, ret,
                                                 (hipStream_t)stream));
}

B747_API int32_t b747_ppo_sample_orders(int64_t *perm, int32_t n_policies, int32_t T, int32_t envs_per_policy, int64_t N,
                                        uint64_t seed, const uint64_t *step_base, uint32_t epoch, void *stream)
{
    const char *const W = "b747_ppo_sample_orders";
    if (int32_t e = check_not_null(W, {{perm, "perm"}})) return e;
    if (T < 0) return bad_arg(W, "T < 0");
    if (int32_t e = check_pop_groups(W, envs_per_policy, n_policies, "n_policies < 1")) return e;
    if ((int64_t)n_policies * envs_per_policy > N)
        return bad_arg(W, "N (fewer envs than n_policies * envs_per_policy: a member's rows would lie outside the rollout)");
    if ((int64_t)T * envs_per_policy > kOrderMaxRows)
        return bad_arg(W, "T * envs_per_policy > 16384 (one workgroup sorts a member's keys in LDS, 8 bytes each)");
    if (T == 0) return 0;
    return launched(W, launch_ppo_sample_orders(perm, n_policies, T, envs_per_policy, N, seed, step_base, epoch,
                                                (hipStream_t)stream));
}

B747_API int32_t b747_ppo_track_best(const double *eval_out, int64_t n_eval, const double *vref, double tk,
                                     int32_t n_members, int32_t envs_per_policy, int32_t n_refs, int32_t window,
                                     int32_t repeat, const float *params, int64_t stride, double *ring, int64_t *count,
                                     double *last, double *window_mean, double *best_quality, int64_t *best_eval,
                                     float *best_params, void *stream)
{
    const char *const W = "b747_ppo_track_best";
    if (int32_t e = check_not_null(W, {{eval_out, "eval_out"}, {vref, "vref"}, {params, "params"}, {ring, "ring"},
                                       {count, "count"}, {last, "last"}, {window_mean, "window_mean"},
                                       {best_quality, "best_quality"}, {best_eval, "best_eval"},
                                       {best_params, "best_params"}}))
        return e;
    if (n_members < 1) return bad_arg(W, "n_members < 1");
    if (envs_per_policy < 64 || envs_per_policy % 64 != 0)
        return bad_arg(W, "envs_per_policy (a positive multiple of 64: the evaluation flies one policy per wave)");
    if (n_refs < 1 || n_refs > envs_per_policy) return bad_arg(W, "n_refs (outside [1, envs_per_policy])");
    if (n_eval < (int64_t)(n_members - 1) * envs_per_policy + n_refs || n_eval > (int64_t)n_members * envs_per_policy)
        return bad_arg(W, "n_eval (outside ((n_members - 1) * envs_per_policy + n_refs - 1, n_members * envs_per_policy])");
    if (window < 1 || window > kTrackMaxWindow)
        return bad_arg(W, "window (outside [1, 128]: NumPy's summation order is kept up to 128 values)");
    if (repeat < 1 || repeat > kTrackMaxRepeat) return bad_arg(W, "repeat (outside [1, 256])");
    if (stride < 4 || stride % 4 != 0)
        return bad_arg(W, "stride (at least 4 floats and a multiple of 4: the snapshot is copied 16 bytes at a time)");
    if (!(tk > 0.0)) return bad_arg(W, "tk (not above 0)");
    const TrackArgs a{eval_out, vref, params, ring, count, last, window_mean, best_quality, best_eval, best_params,
                      n_eval, stride, tk, n_members, envs_per_policy, n_refs, window, repeat};
    return launched(W, launch_ppo_track_best(a, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_exploit(const double *score, int32_t n_members, int32_t n_replace, uint64_t seed,
                                  const uint64_t *step_base, uint32_t round, float *params, int64_t stride,
                                  float *state0, float *state1, int64_t n_state, int64_t *upd_t, double *hyper,
                                  const double *explore, double *rew, int32_t *src_of, void *stream)
{
    const char *const W = "b747_ppo_exploit";
    if (int32_t e = check_not_null(W, {{score, "score"}, {params, "params"}, {state0, "state0"}, {state1, "state1"},
                                       {upd_t, "upd_t"}, {src_of, "src_of"}}))
        return e;
    if (n_members < 2 || n_members > kExploitMaxMembers)
        return bad_arg(W, "n_members (outside [2, 4096]: one workgroup ranks the scores in LDS)");
    if (n_replace < 1 || n_replace > n_members / 2)
        return bad_arg(W, "n_replace (outside [1, n_members / 2]: winners and losers must be disjoint)");
    if (stride < 4 || stride % 4 != 0)
        return bad_arg(W, "stride (at least 4 floats and a multiple of 4: a parameter row is copied 16 bytes at a time)");
    if (n_state < 1) return bad_arg(W, "n_state < 1");
    if (explore && !hyper) return bad_arg(W, "explore without hyper (there is no table to perturb)");
    ExploitArgs a{};
    a.score = score; a.step_base = step_base; a.params = params; a.state0 = state0; a.state1 = state1; a.upd_t = upd_t;
    a.hyper = hyper; a.rew = rew; a.src_of = src_of; a.stride = stride; a.n_state = n_state; a.seed = seed;
    a.round = round; a.n_members = n_members; a.n_replace = n_replace; a.has_explore = explore ? 1 : 0;
    for (int j = 0; j < kExploitCols; ++j) {
        // (a host array, read here; without one the factors are 1 and the bounds open, which the kernel does not read)
        const double f_lo = explore ? explore[4 * j] : 1.0, f_hi = explore ? explore[4 * j + 1] : 1.0;
        const double lo = explore ? explore[4 * j + 2] : -INFINITY, hi = explore ? explore[4 * j + 3] : INFINITY;
        if (!isfinite(f_lo) || !isfinite(f_hi) || !(f_lo > 0.0) || !(f_hi > 0.0))
            return bad_arg(W, "explore (a factor that is not finite and above 0)");
        if (f_lo > f_hi) return bad_arg(W, "explore (f_lo > f_hi)");
        if (lo != lo || hi != hi) return bad_arg(W, "explore (a bound is NaN)");
        if (lo > hi) return bad_arg(W, "explore (min > max)");
        a.explore[j][0] = f_lo; a.explore[j][1] = f_hi; a.explore[j][2] = lo; a.explore[j][3] = hi;
    }
    return launched(W, launch_ppo_exploit(a, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_epoch(float *theta, int32_t obs_dim, const float *obs, const float *act, const float *old_logp,
                                const float *adv, const float *ret, const int64_t *perm, int64_t n_rows,
                                int64_t batch_size, double clip_range, double ent_coef, double vf_coef, void *workspace,
                                float *grad, float *m, float *v, int64_t *t, double max_grad_norm, double lr,
                                double beta1, double beta2, double eps, float *stats, void *stream)
{
    const UpdData d{obs, act, old_logp, adv, ret};
    if (int32_t e = check_upd_policy(nullptr, theta, obs_dim)) return e;
    if (int32_t e = check_upd_rows(nullptr, d, perm, true, n_rows, batch_size, workspace)) return e;
    if (int32_t e = check_not_null(nullptr, {{grad, "grad"}, {m, "m"}, {v, "v"}, {t, "t"}, {stats, "stats"}})) return e;
    return launched("b747_ppo_epoch",
                    launch_ppo_epoch({theta, m, v, t}, obs_dim, d, perm, n_rows, batch_size, {clip_range, ent_coef, vf_coef},
                                     workspace, grad, {max_grad_norm, beta1, beta2, eps}, lr, stats, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_epoch_population(float *theta, int32_t n_policies, int64_t policy_stride, int32_t obs_dim,
                                           const float *obs, const float *act, const float *old_logp, const float *adv,
                                           const float *ret, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                                           double clip_range, double ent_coef, double vf_coef, void *workspace,
                                           float *grad, float *m, float *v, int64_t *t, double max_grad_norm,
                                           const double *lr, double beta1, double beta2, double eps, float *stats,
                                           void *stream)
{
    const char *const W = "b747_ppo_epoch_population";
    const UpdData d{obs, act, old_logp, adv, ret};
    if (int32_t e = check_upd_policy(W, theta, obs_dim)) return e;
    if (int32_t e = check_upd_members(W, n_policies, policy_stride, obs_dim)) return e;
    if (int32_t e = check_upd_rows(W, d, perm, true, n_rows, batch_size, workspace)) return e;
    if (int32_t e = check_not_null(W, {{grad, "grad"}, {m, "m"}, {v, "v"}, {t, "t"}})) return e;
    if (!lr) return bad_arg(W, "lr is NULL (a host array, one learning rate per member)");
    if (!stats) return bad_arg(W, "stats is NULL");
    return launched(W, launch_ppo_epoch_population({theta, m, v, t}, n_policies, policy_stride, obs_dim, d, perm, n_rows,
                                                   batch_size, {clip_range, ent_coef, vf_coef}, workspace, grad,
                                                   {max_grad_norm, beta1, beta2, eps}, lr, stats, (hipStream_t)stream));
}

B747_API int64_t b747_ppo_epoch_batched_workspace(int32_t obs_dim, int64_t batch_size)
{
    if (!policy_obs_dim_ok(obs_dim)) return bad_arg("b747_ppo_epoch_batched_workspace: obs_dim (3, 5, 7, 8 or 10)");
    if (batch_size < 2)
        return bad_arg("b747_ppo_epoch_batched_workspace: batch_size < 2 (the advantages' standard deviation needs two "
                       "rows)");
    return upd_pop_ws_bytes(obs_dim, batch_size);
}

B747_API int32_t b747_ppo_epoch_batched(float *theta, int32_t n_policies, int64_t policy_stride, int32_t obs_dim,
                                        const float *obs, const float *act, const float *old_logp, const float *adv,
                                        const float *ret, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                                        double clip_range, double ent_coef, double vf_coef, void *workspace,
                                        int64_t workspace_bytes, float *m, float *v, int64_t *t, double max_grad_norm,
                                        const double *lr_dev, double beta1, double beta2, double eps, float *stats,
                                        void *stream)
{
    const char *const W = "b747_ppo_epoch_batched";
    const UpdData d{obs, act, old_logp, adv, ret};
    if (int32_t e = check_upd_policy(W, theta, obs_dim)) return e;
    if (int32_t e = check_upd_members(W, n_policies, policy_stride, obs_dim)) return e;
    if (int32_t e = check_upd_rows(W, d, perm, true, n_rows, batch_size, workspace)) return e;
    if (workspace_bytes < upd_pop_ws_bytes(obs_dim, batch_size))
        return bad_arg(W, "workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch_size))");
    if (int32_t e = check_not_null(W, {{m, "m"}, {v, "v"}, {t, "t"}})) return e;
    if (!lr_dev) return bad_arg(W, "lr_dev is NULL (a device array, one learning rate per member)");
    if (!stats) return bad_arg(W, "stats is NULL");
    return launched(W, launch_ppo_epoch_batched({theta, m, v, t}, n_policies, policy_stride, obs_dim, d, perm, n_rows,
                                                batch_size, {clip_range, ent_coef, vf_coef}, workspace, workspace_bytes,
                                                {max_grad_norm, beta1, beta2, eps}, lr_dev, stats, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_epoch_population_hyper(float *theta, int32_t n_policies, int64_t policy_stride,
                                                 int32_t obs_dim, const float *obs, const float *act,
                                                 const float *old_logp, const float *adv, const float *ret,
                                                 const int64_t *perm, int64_t n_rows, int64_t batch_size,
                                                 const double *hyper, void *workspace, float *grad, float *m, float *v,
                                                 int64_t *t, double beta1, double beta2, double eps, float *stats,
                                                 void *stream)
{
    const char *const W = "b747_ppo_epoch_population_hyper";
    const UpdData d{obs, act, old_logp, adv, ret};
    if (int32_t e = check_upd_policy(W, theta, obs_dim)) return e;
    if (int32_t e = check_upd_members(W, n_policies, policy_stride, obs_dim)) return e;
    if (int32_t e = check_upd_rows(W, d, perm, true, n_rows, batch_size, workspace)) return e;
    if (int32_t e = check_not_null(W, {{grad, "grad"}, {m, "m"}, {v, "v"}, {t, "t"}})) return e;
    if (!hyper) return bad_arg(W, "hyper is NULL (a host table, one row of B747_PPO_HYPER_COLS doubles per member)");
    if (!stats) return bad_arg(W, "stats is NULL");
    return launched(W, launch_ppo_epoch_population_hyper({theta, m, v, t}, n_policies, policy_stride, obs_dim, d, perm,
                                                         n_rows, batch_size, hyper, workspace, grad,
                                                         {0.0, beta1, beta2, eps}, stats, (hipStream_t)stream));
}

B747_API int32_t b747_ppo_epoch_batched_hyper(float *theta, int32_t n_policies, int64_t policy_stride, int32_t obs_dim,
                                              const float *obs, const float *act, const float *old_logp,
                                              const float *adv, const float *ret, const int64_t *perm, int64_t n_rows,
                                              int64_t batch_size, const double *hyper_dev, void *workspace,
                                              int64_t workspace_bytes, float *m, float *v, int64_t *t, double beta1,
                                              double beta2, double eps, float *stats, void *stream)
{
    const char *const W = "b747_ppo_epoch_batched_hyper";
    const UpdData d{obs, act, old_logp, adv, ret};
    if (int32_t e = check_upd_policy(W, theta, obs_dim)) return e;
    if (int32_t e = check_upd_members(W, n_policies, policy_stride, obs_dim)) return e;
    if (int32_t e = check_upd_rows(W, d, perm, true, n_rows, batch_size, workspace)) return e;
    if (workspace_bytes < upd_pop_ws_bytes(obs_dim, batch_size))
        return bad_arg(W, "workspace_bytes (below one member's b747_ppo_epoch_batched_workspace(obs_dim, batch_size))");
    if (int32_t e = check_not_null(W, {{m, "m"}, {v, "v"}, {t, "t"}})) return e;
    if (!hyper_dev)
        return bad_arg(W, "hyper_dev is NULL (a device table, one row of B747_PPO_HYPER_COLS doubles per member)");
    if (!stats) return bad_arg(W, "stats is NULL");
    return launched(W, launch_ppo_epoch_batched_hyper({theta, m, v, t}, n_policies, policy_stride, obs_dim, d, perm,
                                                      n_rows, batch_size, hyper_dev, workspace, workspace_bytes,
                                                      {0.0, beta1, beta2, eps}, stats, (hipStream_t)stream));
}

B747_API int32_t b747_consts_default(b747_consts *c)
{
    if (!c) return bad_arg("consts is NULL");
    c->Iz = B747_DEF_IZ;
    c->P = B747_DEF_P;
    c->S = B747_DEF_S;
    c->c_ = B747_DEF_C;
    c->g = B747_DEF_G;
    c->m0 = B747_DEF_M0;
    for (int j = 0; j < 4; ++j) { c->PID_CS[j] = B747_DEF_PID_CS[j]; c->PID_SS[j] = B747_DEF_PID_SS[j]; }
    return 0;
}

B747_API int32_t b747_model_initialize(const b747_model_batch *b, const uint8_t *mask, void *stream)
{
    int32_t r = check_batch(b, false);
    if (r <= 0) return r;
    if (!b->state0) return bad_arg("state0 is NULL");
    with_bools([&](auto x64) {
        hipLaunchKernelGGL(k_model_init<storage_t<decltype(x64)>>, dim3(grid_for(b->n)), dim3(kBlock), 0,
                           (hipStream_t)stream, *b, mask);
    }, b->x_f64 != 0);
    return launched("b747_model_initialize");
}

B747_API int32_t b747_model_step(const b747_model_batch *b, const b747_consts *c, int32_t n_steps, void *stream)
{
    int32_t r = check_batch(b, true);
    if (r <= 0) return r;
    if (!c) return bad_arg("consts is NULL");
    if (n_steps < 0) return bad_arg("n_steps < 0");
    if (n_steps == 0) return 0;
    const Consts C = consts_of(c);
    const ModelPlan p = plan_model(*b, is_default(*c), g_spec, n_steps);
    const bool ok = b->variant != B747_VARIANT_FAITHFUL ? launch_model_step_fast(*b, C, p, n_steps, (hipStream_t)stream)
                                                        : launch_model_step<false>(*b, C, p, n_steps, (hipStream_t)stream);
    if (!ok) return bad_plan("b747_model_step");
    return launched("b747_model_step");
}


B747_API int32_t b747_env_obs_dim(int32_t obs_type)
{
    if (obs_type < 0 || obs_type > 4) return bad_arg("obs_type");
    return obs_dim_of(obs_type);
}

B747_API int32_t b747_env_config_default(b747_env_config *cfg, int32_t obs_type, int32_t reward_type)
{
    if (!cfg) return bad_arg("cfg is NULL");
    memset(cfg, 0, sizeof(*cfg));
    cfg->obs_type = obs_type;
    cfg->reward_type = reward_type;
    cfg->ctrl_type = B747_CTRL_MANUAL;             // main.py:91
    cfg->ctrl_mode = B747_MODE_DIRECT;
    cfg->reset_ref_mode = B747_RESET_CONST;
    cfg->disturbance_mode = B747_DIST_NONE;
    cfg->norm_obs = 1;                             // main.py:15-16
    cfg->norm_act = 1;
    cfg->use_limiter = 0;
    cfg->auto_reset = 1;                           // SB3 VecEnv semantics
    cfg->sample_time = 0.05;                       // main.py:18
    cfg->n_sub = 5;
    cfg->tk = 20.0;                                // main.py:95
    cfg->action_max = 17 * PI / 180;               // Controller default / DIRECT_CONTROL
    cfg->vartheta_max = 10 * PI / 180;
    switch (reward_type) {
    case B747_REW_CLASSIC: {                       // env/ctrl_env.py:112-123
        double k1 = 2, k2 = 2, k3 = 1, s = k1 + k2 + k3;
        cfg->rew[0] = k1 / s; cfg->rew[1] = k2 / s; cfg->rew[2] = k3 / s;
        cfg->rew[3] = 0.1;                         // kf
        cfg->rew[4] = 0.3;                         // kITSE
        cfg->rew[5] = 2;                           // k0
        cfg->rew[6] = -log(0.8) / 10;              // kt = calc_exp_k(0.8, 10), tools/general.py:32
        cfg->rew[7] = -log(0.75) / 0.15;           // ko = calc_exp_k(0.75, 0.15)
        break;
    }
    case B747_REW_PID_LIKE: cfg->rew[0] = 10; break;                       // :146
    case B747_REW_MINIMAL: cfg->rew[0] = 0.2; cfg->rew[1] = 2; cfg->rew[2] = 0.5; break;  // :157-160
    case B747_REW_TF_REFERENCE: cfg->rew[0] = 2; cfg->rew[1] = 5; cfg->rew[2] = 0.1; break;  // :177-179
    default: break;
    }
    cfg->seed = 0;
    return 0;
}

B747_API int32_t b747_env_reset(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                const uint8_t *mask, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r <= 0) return r;
    (void)c;
    with_bools([&](auto x64) {
        hipLaunchKernelGGL(k_env_reset<storage_t<decltype(x64)>>, dim3(grid_for(b->n)), dim3(kBlock), 0,
                           (hipStream_t)stream, *b, *cfg, mask);
    }, b->x_f64 != 0);
    return launched("b747_env_reset");
}

B747_API int32_t b747_env_rollout(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                  const float *actions, int32_t n_env_steps, float *obs_seq, float *reward_seq,
                                  uint8_t *done_seq, void *stream)
{
    int32_t r = check_env(b, cfg);
    if (r <= 0) return r;
    if (!c) return bad_arg("consts is NULL");
    if (!actions) return bad_arg("actions is NULL");
    if (n_env_steps < 0) return bad_arg("n_env_steps < 0");
    if (n_env_steps == 0) return 0;
    const Consts C = consts_of(c);
    hipStream_t s = (hipStream_t)stream;
    const EnvPlan p = plan_env(*b, *cfg, is_default(*c), g_spec, n_env_steps);
    const bool ok = b->variant != B747_VARIANT_FAITHFUL
                        ? launch_env_steps_fast(*b, *cfg, C, p, actions, n_env_steps, obs_seq, reward_seq, done_seq, s)
                        : launch_env_steps<false>(*b, *cfg, C, p, actions, n_env_steps, obs_seq, reward_seq, done_seq, s);
    if (!ok) return bad_plan("b747_env_rollout");
    return launched("b747_env_rollout");
}

B747_API int32_t b747_env_kernel(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                 int32_t n_env_steps)
{
    int32_t r = check_env(b, cfg);
    if (r <= 0) return r < 0 ? r : bad_arg("empty batch");
    if (!c) return bad_arg("consts is NULL");
    return (int32_t)plan_env(*b, *cfg, is_default(*c), g_spec, n_env_steps).kernel;   // b747_env_rollout's plan
}

B747_API int32_t b747_set_specialization(int32_t on)
{
    const int32_t prev = g_spec;
    g_spec = (on == 2) ? 2 : (on ? 1 : 0);
    return prev;
}

B747_API int32_t b747_get_specialization(void) { return g_spec; }

B747_API int32_t b747_env_step(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c, void *stream)
{
    if (b && b->n > 0 && !b->action) return bad_arg("action is NULL");
    return b747_env_rollout(b, cfg, c, b ? b->action : nullptr, 1, nullptr, nullptr, nullptr, stream);
}

B747_API int32_t b747_env_step_seq(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                   const float *actions, int32_t n_env_steps, void *stream)
{
    if (n_env_steps < 0 || (n_env_steps > 0 && !actions)) return bad_arg("actions/n_env_steps");
    for (int32_t t = 0; t < n_env_steps; ++t) {   // one per-step launch each, as n_env_steps b747_env_step calls
        const int32_t rc = b747_env_rollout(b, cfg, c, actions + (int64_t)t * (b ? b->n : 0), 1, nullptr, nullptr,
                                            nullptr, stream);
        if (rc != 0) return rc;
    }
    return 0;
}

B747_API int32_t b747_env_time_steps(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                     const float *actions, int32_t n_env_steps, float *ms_out, void *stream)
{
    if (!ms_out || !actions || n_env_steps <= 0) return bad_arg("actions/ms_out/n_env_steps");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    hipError_t e = hipEventCreateWithFlags(&e0, hipEventDisableSystemFence);
    if (e != hipSuccess) return fail(e, "hipEventCreateWithFlags");
    e = hipEventCreateWithFlags(&e1, hipEventDisableSystemFence);
    if (e != hipSuccess) { (void)hipEventDestroy(e0); return fail(e, "hipEventCreateWithFlags"); }
    int32_t rc = 0;
    for (int32_t t = 0; t < n_env_steps && rc == 0; ++t) {
        (void)hipEventRecord(e0, s);
        rc = b747_env_rollout(b, cfg, c, actions + (int64_t)t * b->n, 1, nullptr, nullptr, nullptr, stream);
        (void)hipEventRecord(e1, s);
        e = hipEventSynchronize(e1);
        if (e != hipSuccess) { rc = fail(e, "hipEventSynchronize"); break; }
        e = hipEventElapsedTime(&ms_out[t], e0, e1);
        if (e != hipSuccess) rc = fail(e, "hipEventElapsedTime");
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

}  // extern "C"
