/* b747.h -- C ABI of libb747.so, the MI355X-native batched B747 pitch-control environment.
 *
 * Drop-in boundary.  The reference drives ONE aircraft per process through the Simulink
 * "exported globals" ABI of core/model_simple_win64.dll via ctypes:
 *     model_simple_initialize()   core/model.py:124 (bound), :238-244 (Model.initialize)
 *     model_simple_step()         core/model.py:125,          :247-250 (Model.step)
 *     model_simple_terminate()    core/model.py:126,          :253-256
 *     parameter / signal globals  core/model.py:129-164 (in_dll bindings)
 * and the env loop on top of it (core/controller.py:134-264, env/ctrl_env.py:237-278).
 * This library replaces that whole chain for N environments at once:
 *   - b747_model_*  : the DLL ABI, batched.  Every exported global becomes a [N] (or [k][N])
 *                     device array; initialize/step act on all envs (or a masked subset).
 *   - b747_env_*    : ControllerEnv.step/reset (obs -> action -> reward -> done, sub-stepping,
 *                     action modes, random resets) fused into one launch per env step.
 * All pointers are DEVICE pointers (e.g. torch.Tensor.data_ptr() of ROCm tensors), laid out
 * structure-of-arrays: field-major, env-minor ("[F][N]").  Every call is asynchronous on the
 * given HIP stream (NULL = default stream) and returns 0 or a negative hipError_t; no call
 * allocates, synchronises or throws.  Calls on different batches are re-entrant; calls on the
 * same batch must be stream-ordered (like the reference, one model instance is not thread-safe).
 */
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B747_ABI_VERSION 15  /* 1: round 1; 2: + b747_set_specialization, b747_policy_*, b747_ppo_rollout;
                                * 3: + b747_env_batch.rec_params, b747_struct_size; 4: + b747_env_batch.ep_stats;
                                * 5: + b747_env_step_seq; 6: b747_model_batch.aero_err is double (the DLL's
                                * `double aero_err[5]`, core/model.py:164), the policy buffer gains the layer-1
                                * matrix-core fragments (b747_policy_num_params); 7: b747_env_batch.aero_err and
                                * .ref are double (the reference's float64 draws and references reach the DLL
                                * unrounded: core/controller.py:153-193); 8: B747_VARIANT_MIXED, and b747_ppo_rollout /
                                * the two-wave kernels run sample_time > dt (n_sub DLL steps per env step); 9: + b747_env_kernel,
                                * and ep_return / ep_final_return accumulate as SB3's VecMonitor (float32); 10:
                                * b747_ppo_rollout advances *step_base by T on the device, b747_env_batch.ep_return is float
                                * (it holds float32 values; 8 B less per env step); 11: + b747_eval_episodes;
                                * 12: + b747_ppo_update_workspace, b747_ppo_grad, b747_ppo_adam; 13: + b747_ppo_gae,
                                * b747_ppo_epoch, b747_get_specialization; 14: + b747_ppo_rollout_lanes; 15: + b747_eval_population,
                                * b747_policy_pack_batch.  b747_ppo_rollout_population, b747_ppo_epoch_population,
                                * b747_ppo_epoch_batched_workspace and b747_ppo_epoch_batched, then
                                * b747_ppo_gae_population, b747_ppo_epoch_population_hyper and b747_ppo_epoch_batched_hyper,
                                * then b747_ppo_sample_orders, then b747_ppo_track_best, then b747_a2c_grad,
                                * b747_ppo_rmsprop and b747_a2c_update, then b747_a2c_update_population, then
                                * b747_ppo_exploit
                                * came later as purely additive entry points under 15 (no struct, argument or
                                * behaviour of an existing one changed): a library built before them still reports
                                * 15, and a binding catches it by the missing entry point (_lib.bind) */

#define B747_NX 18   /* continuous states, SURVEY A.1 (dll.data@0x2b380) */
#define B747_NDISC 9 /* compact discrete state, see b747_model_batch.disc */
#define B747_NSIG 31 /* exported signals, see B747_SIG_* */
#define B747_NAERO 5 /* aero_err components (CXa, CYa, mz, dCm/ddeltaz, K_alpha) */

/* Arithmetic variant of the dynamics (all parity-tested against the oracle):
 *   FAST     fp64: sin/cos(theta) from the quaternion, sin/cos(alpha) from (u, v)/V, pow via exp/log,
 *            reciprocals instead of divisions -- each a few ulp from the DLL's operations;
 *   FAITHFUL fp64: the DLL's operations in the DLL's order (bit-exact vs the CPU oracle on one libm);
 *   MIXED    FAST, except that the two-wave env kernels of the training configuration compute the flight
 *            aerodynamics (ISA atmosphere, speed, alpha, the table lookups, forces, pitching moment) in fp32;
 *            the state, the attitude, the RK4 integration and the whole control side stay fp64.  Per step from
 *            the oracle's state: within 2e-6 |oracle| + 1e-7 + 1e-7 x the batch's largest |value| (absolute ~1e-7
 *            at full scale for the normalised observations and the reward, relative above it); free-running over
 *            a 20 s episode: median deviation 6e-8 of scale, 99th percentile 1.8e-5 (tests/test_gpu_mixed.py,
 *            DESIGN.md 5).  Every other kernel runs FAST.  (round 4, ABI v8) */
#define B747_VARIANT_FAST 0
#define B747_VARIANT_FAITHFUL 1
#define B747_VARIANT_MIXED 2

/* flags[i] bits = the DLL's use_* parameters (each tested as `>= 1.0`, dll@0x1ee9 etc.) */
#define B747_F_PID_SS 1u /* use_PID_SS: SS (pitch) PID drives U_com          */
#define B747_F_PID_CS 2u /* use_PID_CS: CS (altitude) PID drives the pitch reference */
#define B747_F_RP 4u     /* use_RP: actuator model (delay, lag, rate limit, saturation) */
#define B747_F_RL 8u     /* use_RL: PID output with +-10 deg dead zone      */

/* Exported-signal order of b747_model_batch.sig ([B747_NSIG][N] doubles). */
enum {
    B747_SIG_SIM_TIME = 0, B747_SIG_DVARTHETA, B747_SIG_U_COM, B747_SIG_ALPHA, B747_SIG_V,
    B747_SIG_STATE /* 6 entries: x, y, Vx, Vy, vartheta, wz */,
    B747_SIG_MACH = B747_SIG_STATE + 6, B747_SIG_DVARTHETA_DT, B747_SIG_DVARTHETA_DT_DT,
    B747_SIG_DVARTHETA_INT, B747_SIG_AE, B747_SIG_ITAE, B747_SIG_IAE, B747_SIG_ISE, B747_SIG_ITSE,
    B747_SIG_SE, B747_SIG_TAE, B747_SIG_TSE, B747_SIG_K_ALPHA, B747_SIG_MZ, B747_SIG_DCM_DDELTAZ,
    B747_SIG_CXA, B747_SIG_CYA, B747_SIG_DELTAZ_RP, B747_SIG_U_COM_PID, B747_SIG_VARTHETA_ZH
};

/* Batch-wide model parameters (the DLL's scalar model parameters, dll.data@0x24000...). */
typedef struct b747_consts {
    double Iz, P, S, c_, g, m0;
    double PID_CS[4]; /* [Kp, Ki, Kd, N] of the CS (altitude-hold) loop */
    double PID_SS[4]; /* [Kp, Ki, Kd, N] of the SS (pitch-stabilisation) loop */
} b747_consts;

/* One batch of N independent models = N copies of the reference DLL's static data.
 * State (read+write):
 *   X     [18][N]  float (x_f64 == 0) or double (x_f64 == 1): continuous states, SURVEY A.1
 *   disc  [9][N]   double: x_dss, y_dss (held), rate-limiter PrevY, Derivative inputs at the
 *                  last major step (dvartheta, dvartheta_dt), U_com history (slot j&3 = step j)
 *   k     [N]      uint32: major step counter (time = k * 0.01 s)
 *   mem   [N]      uint8 : anti-windup Memory blocks (bit0 SS loop, bit1 CS loop)
 * Parameters (read):
 *   deltaz, vartheta, h_zh [N] double; flags [N] uint8 (B747_F_*); aero_err [5][N] double (the DLL's
 *   parameter precision: core/model.py:164 binds `(real_T*5).in_dll(dll, "aero_err")`, real_T = c_double);
 *   state0 [6][N] double (read by initialize only)
 * Read-out (write, nullable): sig [31][N] double = every exported signal after the call, i.e.
 *   what core/model.py's properties return after Model.step()/initialize(). */
typedef struct b747_model_batch {
    int64_t n;
    int32_t x_f64;
    int32_t variant;   /* B747_VARIANT_FAST (0, default), B747_VARIANT_FAITHFUL (MIXED runs FAST here) */
    void *X;
    double *disc;
    uint32_t *k;
    uint8_t *mem;
    const double *deltaz;
    const double *vartheta;
    const double *h_zh;
    const uint8_t *flags;
    const double *aero_err;
    const double *state0;
    double *sig;
} b747_model_batch;

/* ABI version (B747_ABI_VERSION) -- lets a ctypes binding check it loaded the right library. */
int32_t b747_abi_version(void);
/* sizeof of the ABI structs (B747_STRUCT_*), or -1: a binding checks its struct mirrors against these. */
enum { B747_STRUCT_CONSTS = 0, B747_STRUCT_MODEL_BATCH = 1, B747_STRUCT_ENV_CONFIG = 2, B747_STRUCT_ENV_BATCH = 3 };
int64_t b747_struct_size(int32_t which);
/* Fill *c with the DLL's defaults (Iz = 6.73e7, P = 275000, PID gains, ...). */
int32_t b747_consts_default(b747_consts *c);

/* model_simple_initialize (dll@0x12a0) for every env with mask[i] != 0 (mask NULL = all).
 * Replaces core/model.py:238-241.  Signals (if sig != NULL) are zeroed, as in the DLL. */
int32_t b747_model_initialize(const b747_model_batch *b, const uint8_t *mask, void *stream);

/* n_steps consecutive model_simple_step calls (dll@0x16d0) on every env: one ode4 step of
 * h = 0.01 s each.  Replaces core/model.py:247-250 (x N envs, x n_steps).  n_steps = 1 with the DLL's
 * default constants (FAST) runs each env over three waves (k_model_step_split), and so does n_steps > 1 for up
 * to 16,384 envs, with the state in registers across the steps (k_model_steps_split); otherwise -- larger batches,
 * other constants, FAITHFUL -- one wave per env with the state in registers across the n_steps (k_model_step): the
 * same operations, agreeing to a few ulp (FMA contraction); b747_set_specialization(0) keeps every call on the
 * one-wave kernel. */
int32_t b747_model_step(const b747_model_batch *b, const b747_consts *c, int32_t n_steps,
                        void *stream);

/* ------------------------------------------------------------------ env level ---------
 * ControllerEnv (env/ctrl_env.py) + Controller (core/controller.py) for N envs.
 * Enum values equal the reference's Python Enum values. */
enum { B747_OBS_PID_LIKE = 0, B747_OBS_SPEED_MODE = 1, B747_OBS_PID_AERO = 2,
       B747_OBS_PID_SPEED_AERO = 3, B747_OBS_MODEL_STATE = 4 };
enum { B747_REW_CLASSIC = 0, B747_REW_PID_LIKE = 1, B747_REW_QUALITY = 2, B747_REW_MINIMAL = 3,
       B747_REW_TF_REFERENCE = 4 };
enum { B747_CTRL_FULL_AUTO = 0, B747_CTRL_AUTO = 1, B747_CTRL_SEMI_MANUAL = 2, B747_CTRL_MANUAL = 3 };
enum { B747_MODE_NONE = -1, B747_MODE_DIRECT = 0, B747_MODE_ADD_PROC = 1, B747_MODE_ANG_VEL = 2,
       B747_MODE_ADD_DIRECT = 3 };
enum { B747_RESET_NONE = -1, B747_RESET_CONST = 0, B747_RESET_OSCILLATING = 1, B747_RESET_HYBRID = 2 };
enum { B747_DIST_NONE = -1, B747_DIST_AERO = 0 };
enum { B747_REF_CONST = 0, B747_REF_OSC = 1 };

/* Batch-wide env configuration = the ControllerEnv(...) / Controller(...) constructor args. */
typedef struct b747_env_config {
    int32_t obs_type, reward_type, ctrl_type, ctrl_mode, reset_ref_mode, disturbance_mode;
    int32_t norm_obs, norm_act, use_limiter, auto_reset;
    int32_t n_sub;        /* DLL steps per env step: round(sample_time / 0.01) */
    int32_t aero_fixed;   /* AERO disturbance with the fixed vector aero_err_fixed */
    double sample_time, tk, action_max, vartheta_max;
    double rew[8];        /* reward constants (b747_env_config_default documents each type) */
    double aero_err_fixed[5];
    uint64_t seed;        /* Philox key of the random resets */
} b747_env_config;

/* N environments.  Model state as in b747_model_batch, plus the controller's per-env state.
 * obs / terminal_obs are row-major [N][obs_dim] (what a policy consumes). */
typedef struct b747_env_batch {
    int64_t n;
    int64_t env_offset;   /* global id of env 0 (GPU shard offset); RNG stream = seed x global id */
    int32_t x_f64, obs_dim;
    int32_t variant;      /* B747_VARIANT_* */
    int32_t reserved;
    void *X; double *disc; uint32_t *k; uint8_t *mem;
    double *deltaz;       /* DLL parameter deltaz: read/written by a step only in ANG_VEL mode
                           * (the one mode that integrates it; the others derive it from the action) */
    /* The next four are controller-internal slots.  A step reads/writes each only where the
     * configuration uses it (keeps the per-step HBM traffic to what the path needs):
     *   vartheta  written by resets only: a step recomputes it (CS PID on: the 0 that
     *             Model.initialize wrote; off: the pitch reference at t)
     *   h_zh      read every step, written where the CS PID is on (it persists); ref[7] is read
 *             only when the configuration can turn the CS PID on
     *   upid      only in ADD_PROC / ADD_DIRECT ctrl modes
     *   tp        only with the TF_REFERENCE reward                                        */
    double *vartheta;     /* DLL parameter vartheta */
    double *h_zh;         /* DLL parameter h_zh */
    double *upid;         /* U_com_PID read-out of the last step (Model.deltaz_ref) */
    double *tp;           /* TF_REFERENCE reward state */
    uint8_t *flags;       /* B747_F_* per env (HYBRID resets switch the CS PID per env) */
    double *aero_err;     /* [5][N]: the DLL's double aero_err[5] (core/model.py:164), which Controller.reset
                           * fills with float64 normal draws (core/controller.py:181-193) */
    double *ref;          /* [8][N], float64 as the reference's Python floats (core/controller.py:153-177):
                           * [0] const pitch, [1..3] A1..A3, [4..6] f1..f3 (Hz), [7] altitude;
                           * a step reads [0], [7], and [1..6] when the reset mode can give
                           * oscillating references (OSCILLATING or NONE) */
    uint8_t *ref_kind;    /* B747_REF_*; read by a step only when the reset mode can give oscillating
                           * references (OSCILLATING or NONE): CONST / HYBRID treat every ref as constant */
    double *state0;       /* [6][N] initial state used when reset_ref_mode == NONE */
    uint32_t *episode;    /* resets done so far (Philox counter) */
    float *ep_return; int32_t *ep_len;               /* running episode statistics: the return accumulated as
                                                      * SB3's VecMonitor does (float32(return + float64 reward)
                                                      * per step; float since ABI 10); a step derives ep_len from k
                                                      * (ceil(k / n_sub)), resets write it */
    double *ep_final_return; int32_t *ep_final_len;  /* written where done (VecMonitor's episode "r", "l") */
    const float *action;  /* [N] action (action dim 1) */
    float *obs;           /* [N][obs_dim] */
    float *reward;        /* [N] */
    uint8_t *done;        /* [N] */
    float *terminal_obs;  /* [N][obs_dim], nullable: last obs of an episode that ended */
    double *sig;          /* [n_sub][31][N], nullable: every exported signal (B747_SIG_* rows)
                           * after each DLL step of the env step -- what Controller._post_step
                           * records into its Storage (core/controller.py:209-228) and what
                           * core/model.py's properties read; slot q = DLL step q of the env
                           * step (slots before an unaligned first step are left untouched);
                           * for an env that finished, the values before its auto-reset */
    double *rec_params;   /* [3][N], nullable, written only with sig: the DLL parameters vartheta, h_zh
                           * and deltaz in effect during the last env step (before an auto-reset) --
                           * the Controller values _post_step records beside the signals
                           * (vartheta_ref when the CS PID is off, hzh; core/controller.py:209-228) */
    double *ep_stats;     /* [3][N], nullable: per-env episode accumulators, added to where an episode ends
                           * (a step's done): [0] += 1, [1] += its return, [2] += its length -- what SB3's
                           * VecMonitor logs (neural/agent.py:63-82 wraps the env in it), kept on the device
                           * so a caller can reduce them across envs and ranks every M steps
                           * instead of copying every step's info to the host */
} b747_env_batch;

/* Defaults of ControllerEnv/Controller for the given obs/reward types (reward constants of
 * env/ctrl_env.py:109-192 with reward_config = {}; main.py settings for the rest). */
int32_t b747_env_config_default(b747_env_config *cfg, int32_t obs_type, int32_t reward_type);
int32_t b747_env_obs_dim(int32_t obs_type);

/* ControllerEnv.reset (env/ctrl_env.py:273-278) for envs with mask[i] != 0 (NULL = all):
 * random ICs / reference / aero errors per the config, Model.initialize, obs <- zeros. */
int32_t b747_env_reset(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                       const uint8_t *mask, void *stream);

/* ControllerEnv.step (env/ctrl_env.py:260-270) for every env, fused in one launch: action
 * scaling, command injection, action mode, round(sample_time/dt) DLL steps, obs, reward,
 * done, and (auto_reset) the SB3 VecEnv auto-reset with terminal_obs. */
int32_t b747_env_step(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                      void *stream);

/* n_env_steps consecutive env steps in ONE launch with actions[t][N] given up front (open-loop
 * or pre-sampled actions; obs/reward/done of every step are written to obs_seq[t][N][obs_dim],
 * reward_seq[t][N], done_seq[t][N], each nullable).  State stays in registers between steps. */
int32_t b747_env_rollout(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                         const float *actions, int32_t n_env_steps, float *obs_seq, float *reward_seq,
                         uint8_t *done_seq, void *stream);

/* n_env_steps consecutive ControllerEnv.step calls with actions[t][N] given up front, as n_env_steps
 * launches of the per-step kernel (the b747_env_step launch, one per step: the same kernel and the
 * same results as a host loop of b747_env_step with b->action = actions + t*N); obs/reward/done and
 * the episode buffers hold the last step's.  Stream-ordered and graph-capturable; what it saves
 * over such a loop, or over a replayed graph of it, is host-side latency only. */
int32_t b747_env_step_seq(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                          const float *actions, int32_t n_env_steps, void *stream);

/* Measurement helper (synchronous; not for graph capture): runs n_env_steps b747_env_step
 * launches on `stream` (actions[t][N]) with a HIP event pair recorded directly around each
 * launch (events created with hipEventDisableSystemFence so they add no cache flush), and
 * writes each launch's duration in milliseconds to ms_out[t] (host memory). */
int32_t b747_env_time_steps(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                            const float *actions, int32_t n_env_steps, float *ms_out, void *stream);

/* Kernel specialisation switch (diagnostic; process-wide, not thread-safe).  With on != 0 (the
 * default) an env step whose configuration has the branch-selecting fields of the reference's
 * training setup (PID_LIKE obs, CLASSIC reward, MANUAL/DIRECT control, CONST resets, drawn AERO
 * errors, normalised obs/action, no limiter, auto-reset) and the DLL's default constants runs a
 * kernel compiled for exactly that configuration; with on == 1 a single step of it (sample_time = dt)
 * runs each env over three waves (flight / ahead / control), on == 2 keeps one wave per env (the env kernels only:
 * b747_model_step treats 2 as 1); on == 0 forces the generic kernel (tests compare them) and keeps every
 * b747_model_step call on the one-wave kernel.
 * Returns the previous setting.  No reference counterpart (the reference has no kernels). */
int32_t b747_set_specialization(int32_t on);
/* The current setting (0, 1 or 2: what b747_set_specialization last set, 1 at load); changes nothing (ABI 13). */
int32_t b747_get_specialization(void);

/* Which kernel b747_env_rollout(b, cfg, c, ..., n_env_steps) launches for this batch and configuration (b747_env_step
 * is n_env_steps = 1): B747_KERNEL_* below.  Lets a caller (and the tests) confirm that a configuration runs the
 * two-wave kernels of the bench.  No reference counterpart.  Returns < 0 on a bad argument. */
#define B747_KERNEL_GENERIC 0        /* k_env_steps, run-time constants */
#define B747_KERNEL_DEFC 1           /* k_env_steps, the DLL's default constants as literals */
#define B747_KERNEL_RECORDING 2      /* k_env_steps with per-DLL-step signal recording (b747_env_batch.sig) */
#define B747_KERNEL_SPEC_ONE_WAVE 3  /* k_env_steps specialised on the training configuration, one wave per env */
#define B747_KERNEL_STEP_SPLIT 4     /* k_env_step_split: the per-step two-wave kernel (the bench headline) */
#define B747_KERNEL_ROLLOUT_SPLIT 5  /* k_rollout_split<false>: K env steps / n_sub DLL steps, two waves per env */
int32_t b747_env_kernel(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c, int32_t n_env_steps);

/* ---- on-GPU PPO rollout (BASELINE config 5) ----
 * One step of stable-baselines3's collect_rollouts for every env (neural/agent.py:167-171 ->
 * SB3 1.4 PPO.collect_rollouts with the default MlpPolicy): policy forward through separate
 * pi / vf extractors [64, 64] tanh, Gaussian sample with a state-independent log_std, log-prob,
 * value, and the clipped action handed to the env.  params = the policy's parameters flattened
 * in this order (torch Linear weights are [out][in] row-major): pi_net.0.{weight,bias},
 * pi_net.2.{weight,bias}, vf_net.0.{weight,bias}, vf_net.2.{weight,bias}, action_net.{weight,bias},
 * value_net.{weight,bias}, log_std -- fp32, device memory (b747_rl_ctrl_amd/ppo.py flat_params),
 * followed by 2 x 4096 floats that b747_policy_pack fills with the 64x64 layers (scaled by -4/ln 2)
 * repacked for the matrix cores as f16 hi/lo pairs, 2*64*(obs_dim+1) + 4*64 + 3 floats of
 * derived parameters with tanh's scale and affine part folded in, and (from a 16-byte boundary) 1024
 * floats of layer-1 matrix-core fragments (obs_dim <= 4: the first layer of both heads as one
 * v_mfma_f32_32x32x16_f16 per 32-unit tile, its f16 hi/lo split and bias folded into K) -- call it after
 * every parameter update; b747_policy_num_params counts all four parts.  Outputs agree with the float64 policy
 * within 16 times the f32 torch policy's own error plus 2^-22 of the output's scale (f16 hi/lo split products;
 * DESIGN.md "Policy forward against float64", tests/test_gpu_policy_forward_f64.py). */
int32_t b747_policy_num_params(int32_t obs_dim);
/* T rollout steps (policy forward + sample + clip + env step, as b747_policy_act followed by
 * b747_env_step with the same Philox noise) for every env in ONE launch -- each env on two waves, the policy
 * head on one beside the other's RK4 stages, the env state and observation kept in registers across steps --
 * then ONE batched launch of the value head over the T*N rows of obs_buf into val_buf; both on `stream`
 * (SB3 collect_rollouts, neural/agent.py:167-171 -> PPO.collect_rollouts).  Row t*N + i of obs_buf[T][N][3], act_buf, logp_buf, val_buf, rew_buf,
 * done_buf; the env's obs / reward / done hold the last step's afterwards.  Covers the reference's
 * training configuration only (default constants; PID_LIKE, CLASSIC, MANUAL/DIRECT, CONST resets,
 * AERO errors, normalised obs/action, no limiter, auto-reset; fp64 state; FAST; N % 64 == 0) and
 * returns -hipErrorInvalidValue for anything else.  step_base (device, nullable = 0): the Philox counter base of
 * step 0, read by the rollout and advanced by T on the device after it (ABI 10), so that consecutive calls -- or
 * replays of one captured graph -- draw fresh noise with no host or extra kernel in between. */
int32_t b747_ppo_rollout(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c, const float *params,
                         uint64_t seed, uint64_t *step_base, int32_t T, float *obs_buf, float *act_buf,
                         float *logp_buf, float *val_buf, float *rew_buf, uint8_t *done_buf, float act_lo, float act_hi,
                         void *stream);
/* The same T rollout steps in ONE launch for every other env (ABI 14): the arguments of b747_ppo_rollout, with
 * obs_buf [T][N][obs_dim].  Each env on one lane of a one-wave workgroup (64 envs per wave, any N >= 1): the policy
 * with both heads, b747_policy_act's Philox sample (seed, env_offset + i, *step_base + t), log-prob and clip, then the
 * generic lane code of b747_env_step -- every control type / mode, reward, reset mode, disturbance, limiter setting and
 * n_sub, run-time constants, FAST or FAITHFUL arithmetic (MIXED runs FAST) -- with the env state and the observation
 * in registers across the T steps.  Row t*N + i of obs_buf (the observation the policy saw), act_buf (unclipped),
 * logp_buf, val_buf, rew_buf, done_buf.  An episode that ends is booked and, with cfg->auto_reset, reset as
 * b747_env_step does it (terminal_obs, ep_final_*, ep_stats, state0); afterwards the env -- state, obs, reward, done,
 * action (where non-NULL: the last clipped action) -- is what T calls of b747_policy_act + b747_env_step would have
 * left: bit for bit in FAITHFUL, within the FAST kernels' contraction otherwise (tests/test_gpu_ppo_rollout_lanes.py).
 * A second launch then advances *step_base (device, nullable = 0) by T, so that consecutive calls -- or replays of
 * one captured graph -- draw fresh noise: for obs_dim 3 it is b747_ppo_rollout's batched value pass over the T*N rows
 * of obs_buf, which writes val_buf (the value head is then not in the step loop); for obs_dim 5, whose value head
 * runs in the loop, a one-thread launch.  Returns -hipErrorInvalidValue, with the reason in
 * b747_last_error, for an obs_dim other than 3 / 5 (PID_LIKE / SPEED_MODE: the matrix-core policy of the evaluation
 * kernel), fp32 state (x_f64 == 0), a batch that records signals (b->sig), a NULL buffer, T < 0 or act_lo > act_hi;
 * b747_ppo_rollout keeps refusing what it refused before.  T == 0 validates and launches nothing.  Stream-ordered,
 * graph-capturable, no allocation. */
int32_t b747_ppo_rollout_lanes(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                               const float *params, uint64_t seed, uint64_t *step_base, int32_t T, float *obs_buf,
                               float *act_buf, float *logp_buf, float *val_buf, float *rew_buf, uint8_t *done_buf,
                               float act_lo, float act_hi, void *stream);
/* P learners' rollouts side by side in ONE launch (additive under ABI 15): b747_ppo_rollout_lanes with a policy and
 * reward constants per group of envs; everything not named here -- the rows, the Philox counters (seed, env_offset + i,
 * *step_base + t), the episode books and auto-reset, what is left in the env, the configurations covered -- is as
 * above.  params [n_policies][policy_stride] floats: policy p (packed by b747_policy_pack or b747_policy_pack_batch)
 * starts at params + p * policy_stride and flies envs [p * envs_per_policy, (p + 1) * envs_per_policy); the last group
 * may be partial.  envs_per_policy is a positive multiple of 64: each 64-env wave reads one policy, at a wave-uniform
 * address.  rew_pop (nullable, [n_policies][8] double in cfg->rew order): group p's envs are rewarded with rew_pop[p]
 * in place of cfg->rew; only the reward reads them, resets do not.  The value head runs in the step loop for both
 * obs_dims (the batched value pass takes one policy for all rows), and a one-thread launch then advances *step_base by
 * T.  last_val (nullable, [N] float): the value head once more on the observation the rollout ends on (the one left in
 * b->obs) -- the bootstrap value of b747_ppo_gae, the bits of b747_policy_act's value_out on that observation.  With
 * n_policies == 1 and rew_pop == NULL every buffer is b747_ppo_rollout_lanes' bit for bit, except val_buf for obs_dim
 * 3 in FAST (the in-loop head against the batched pass: within the FAST kernels' contraction).  Returns
 * -hipErrorInvalidValue, with the field named in b747_last_error and before any launch, for everything
 * b747_ppo_rollout_lanes refuses and for envs_per_policy not a positive multiple of 64, n_policies < 1, N outside
 * ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy], policy_stride below
 * b747_policy_num_params(obs_dim) or not a multiple of 4.  T == 0 validates and launches nothing.  Stream-ordered,
 * graph-capturable, no allocation. */
int32_t b747_ppo_rollout_population(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                                    const float *params /* [n_policies][policy_stride] */, int32_t n_policies,
                                    int64_t policy_stride /* floats */, int32_t envs_per_policy,
                                    const double *rew_pop /* [n_policies][8], NULL = cfg->rew */,
                                    uint64_t seed, uint64_t *step_base, int32_t T, float *obs_buf, float *act_buf,
                                    float *logp_buf, float *val_buf, float *rew_buf, uint8_t *done_buf,
                                    float *last_val /* [N], nullable */, float act_lo, float act_hi, void *stream);
int32_t b747_policy_pack(float *params, int32_t obs_dim, void *stream);
/* noise [N] (nullable): standard-normal draws; NULL = Philox4x32-10 keyed by seed with counter
 * (env_offset + i, *step_base + step); step_base (device, nullable = 0) lets a captured rollout
 * graph draw fresh noise on every replay.  obs_out (nullable) receives a copy of obs. */
int32_t b747_policy_act(const float *params, int32_t obs_dim, int64_t n, const float *obs, const float *noise,
                        uint64_t seed, const uint64_t *step_base, uint32_t step, int64_t env_offset,
                        float *obs_out, float *act_out,
                        float *logp_out, float *value_out, float *env_action, float act_lo, float act_hi,
                        void *stream);

/* ---- whole evaluation episodes in one launch (ControlTestCallback.calc_stepinfo, neural/callbacks.py:60-100) ----
 * Every env flies one episode from its current state: up to n_env_steps env steps, ending at its first done
 * (t >= tk, or the limiter); from then on the env is frozen -- its stored state is the state at that done -- while
 * the launch goes on for the others.  The action of a step is the policy's mean (params: the buffer b747_policy_pack
 * filled; the policy head only, no noise) on the env's observation, clipped to [act_lo, act_hi] (step 0 reads
 * b->obs); with params == NULL it is b->action[i], held for the whole episode (ignored where the SS PID flies:
 * the PID baseline; an open-loop elevator step otherwise).  After every DLL step (n_sub per env step) the sample
 * scale * nan_to_num(signal sig_row) at sim_time goes into a per-env running calc_stepinfo (tools/general.py:46-61)
 * against y_base[i] with the given error band; no history is kept.  eval_out [B747_NEVAL][N] (double): overshoot (%,
 * signed; NaN if y_base == 0), rise_time, settling_time (s; NaN if none), static_error, the ITSE signal at the end,
 * the episode's length in DLL steps, and the episode return (VecMonitor's float32 accumulation, from b->ep_return).
 * obs / reward / done, terminal_obs (where non-NULL, written at the done), ep_return and the ep_final_* / ep_stats
 * buffers are left as a step loop would leave them at the env's last step, with a policy or without (obs_dim entries
 * per row, any observation type).  One wave per 64 envs on the generic lane code (every configuration b747_env_step
 * covers, run-time constants, FAST or FAITHFUL arithmetic; MIXED runs FAST).  Returns -hipErrorInvalidValue for fp32
 * state (x_f64 == 0), cfg->auto_reset != 0, or a policy with an obs_dim other than 3 / 5.  n_env_steps == 0 validates
 * and launches nothing.  Stream-ordered, graph-capturable, no allocation. */
#define B747_NEVAL 7  /* rows of eval_out: overshoot, rise_time, settling_time, static_error,
                         ITSE at the end, length in DLL steps, episode return */
int32_t b747_eval_episodes(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                           const float *params /* packed by b747_policy_pack; NULL = no policy */,
                           int32_t n_env_steps, int32_t sig_row, double scale, const double *y_base /* [N] */,
                           double error_band, float act_lo, float act_hi,
                           double *eval_out /* [B747_NEVAL][N] */, void *stream);

/* ---- a population of policies and PID gain sets scored in one launch (ABI 15) ----
 * b747_eval_episodes with a policy per group of envs and PID gains per env; everything not named here -- the episode
 * semantics and frozen envs, eval_out, what is left in the batch, the configurations covered -- is as above.
 * params [n_policies][policy_stride] floats: policy p (packed by b747_policy_pack or b747_policy_pack_batch) starts at
 * params + p * policy_stride and flies envs [p * envs_per_policy, (p + 1) * envs_per_policy); the last group may be
 * partial.  envs_per_policy is a positive multiple of 64: each 64-env wave reads one policy, at a wave-uniform address.
 * params == NULL (n_policies 0): no policy, b->action held, as above.  pid_ss / pid_cs (each nullable, [4][N] double,
 * component-major as every batch field): env i flies with PID_SS[j] = pid_ss[j * N + i] (PID_CS likewise) in place of
 * c->PID_SS; a NULL pointer keeps the batch constant.  The gains enter the control law only; resets do not read them.
 * With n_policies == 1 and both gain pointers NULL the result is b747_eval_episodes' bit for bit.  Returns
 * -hipErrorInvalidValue, with the field named in b747_last_error and before any launch, for everything
 * b747_eval_episodes refuses and, with params set, for envs_per_policy not a positive multiple of 64, n_policies < 1,
 * N outside ((n_policies - 1) * envs_per_policy, n_policies * envs_per_policy], policy_stride below
 * b747_policy_num_params(obs_dim) or not a multiple of 4 (the matrix-core fragments start on a 16-byte boundary);
 * with params == NULL for n_policies != 0.  n_env_steps == 0 validates and launches nothing.  Stream-ordered,
 * graph-capturable, no allocation. */
int32_t b747_eval_population(const b747_env_batch *b, const b747_env_config *cfg, const b747_consts *c,
                             const float *params /* [n_policies][policy_stride], NULL = no policy */,
                             int32_t n_policies, int64_t policy_stride /* floats */, int32_t envs_per_policy,
                             const double *pid_ss /* [4][N], NULL = c->PID_SS */,
                             const double *pid_cs /* [4][N], NULL = c->PID_CS */,
                             int32_t n_env_steps, int32_t sig_row, double scale, const double *y_base, double error_band,
                             float act_lo, float act_hi, double *eval_out /* [B747_NEVAL][N] */, void *stream);
/* b747_policy_pack for n_policies parameter sets in ONE launch: set p occupies params + p * policy_stride (its flat
 * parameters first, as for b747_policy_pack; policy_stride >= b747_policy_num_params(obs_dim), a multiple of 4, at most
 * 65535 sets).  Floats of a stride past b747_policy_num_params are not touched. */
int32_t b747_policy_pack_batch(float *params, int32_t obs_dim, int32_t n_policies, int64_t policy_stride, void *stream);

/* ---- one PPO minibatch update on the device (b747_rl_ctrl_amd/ppo.py PPO._minibatch; SB3 1.4 PPO.train) ----
 * For the policy of b747_policy_act (pi / vf nets obs_dim -> 64 -> 64 tanh, action_net, value_net, log_std; obs_dim 3, 5,
 * 7, 8 or 10; one action).  theta = the first P = 128 obs_dim + 8579 floats of the policy buffer, in the order given
 * above (b747_policy_pack is NOT needed between updates, only before the rollout kernels read the buffer again).
 * Two calls per minibatch, so that a data-parallel all-reduce of the one flat gradient fits between them; both are
 * stream-ordered and graph-capturable, allocate nothing, synchronise nothing and use no floating-point atomics: the
 * same inputs give the same bits.  All pointers are device memory.
 *
 * b747_ppo_grad: for the rows r = idx[0 .. batch) (int64 row numbers t * N + i into the time-major rollout buffers
 * obs [T*N][obs_dim], act, old_logp, adv, ret [T*N]) the loss
 *   mean(-min(A ratio, A clamp(ratio, 1 - clip_range, 1 + clip_range))) + ent_coef (-entropy) + vf_coef mean((ret - value)^2)
 * with A = (adv - mean) / (std + 1e-8) over the minibatch (unbiased std, fp64 sums) and ratio = exp(logp - old_logp);
 * grad [P] = its gradient (flat_params order; where the clipped term is strictly smaller the row's policy gradient is
 * 0); stats [8] = the policy-gradient loss, the value loss, the entropy loss, the clip fraction, approx_kl =
 * mean((ratio - 1) - log ratio), mean |A ratio|, mean(|ratio| + 1 + |log ratio|), and the loss.  The forward in fp64, the
 * backward products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: an fp32 fmaf chain), sums over rows in fp32 per
 * workgroup and fp64 across them.  workspace: b747_ppo_update_workspace(obs_dim) bytes, 16-byte aligned, the caller's; its contents mean nothing
 * between calls.  batch >= 2.
 * b747_ppo_adam: g = grad_scale grad (1 / world for data-parallel ranks after a SUM all-reduce); coef = min(1,
 * max_grad_norm / (|g|_2 + 1e-6)) (torch clip_grad_norm_); *t += 1; torch.optim.Adam's update of theta, m, v [n_params]
 * with g coef (bias-corrected, no weight decay; PPO uses betas 0.9 / 0.999, eps 1e-5).  t: one device int64, the
 * number of steps taken so far, advanced by the kernel.  grad is not modified.
 * Both return -hipErrorInvalidValue, before anything reaches the device, for a NULL pointer, an obs_dim that
 * b747_policy_act does not take, batch < 2 or n_params < 1 (b747_last_error names the argument). */
int64_t b747_ppo_update_workspace(int32_t obs_dim);   /* bytes; -hipErrorInvalidValue for an unsupported obs_dim */
int32_t b747_ppo_grad(const float *theta, int32_t obs_dim, const float *obs, const float *act, const float *old_logp,
                      const float *adv, const float *ret, const int64_t *idx, int64_t batch, double clip_range,
                      double ent_coef, double vf_coef, void *workspace, float *grad, float *stats, void *stream);
int32_t b747_ppo_adam(float *theta, float *m, float *v, int64_t *t, const float *grad, int64_t n_params,
                      double grad_scale, double max_grad_norm, double lr, double beta1, double beta2, double eps,
                      void *stream);

/* ---- every minibatch of one PPO epoch from one call (ABI 13; PPO.train's inner loop) ----
 * For j = 0 .. ceil(n_rows / batch_size) - 1: the launches of b747_ppo_grad with idx = perm + j batch_size, batch =
 * min(batch_size, n_rows - j batch_size) and stats + 8 j, then those of b747_ppo_adam with grad_scale 1 and n_params = P
 * -- the same kernels with the same arguments in the same order as the two calls in a host loop, so the same bits; the
 * host work per minibatch is four launches and nothing else (the gradient kernel's LDS limit is raised once per call).
 * perm [n_rows]: int64 row numbers into the rollout buffers (one epoch's permutation); stats [ceil(n_rows /
 * batch_size)][8], one row per minibatch.  Single rank only: a data-parallel all-reduce belongs between the two calls
 * of the two-call path.  Everything is validated before the first launch: the checks of b747_ppo_grad and
 * b747_ppo_adam, n_rows >= 2, batch_size >= 2, and n_rows % batch_size != 1 (a last minibatch of one row has no
 * advantage standard deviation); -hipErrorInvalidValue with the argument named in b747_last_error.  If a launch fails
 * at minibatch j the call returns that error at once and minibatches 0 .. j-1 stay applied to theta, m, v and *t.
 * Stream-ordered, graph-capturable (the capture then holds this perm's addresses), no allocation. */
int32_t b747_ppo_epoch(float *theta, int32_t obs_dim, const float *obs, const float *act, const float *old_logp,
                       const float *adv, const float *ret, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                       double clip_range, double ent_coef, double vf_coef, void *workspace, float *grad,
                       float *m, float *v, int64_t *t, double max_grad_norm, double lr, double beta1, double beta2,
                       double eps, float *stats /* [ceil(n_rows / batch_size)][8] */, void *stream);
/* One epoch for each of n_policies learners from one call (additive under ABI 15): a host loop over the members of
 * b747_ppo_epoch's launches -- the same kernels with the same arguments in the same order, so the same bits -- with
 * member p's theta + p * policy_stride, m / v + p * P, t + p, perm + p * n_rows, lr[p] (a HOST array) and stats + p *
 * ceil(n_rows / batch_size) * 8.  The rollout buffers are shared: member p's perm row holds global row numbers (for
 * b747_ppo_rollout_population's layout, t * N + p * envs_per_policy + j).  grad [P] and workspace are reused by every
 * member.  Everything is validated for every member before the first launch: b747_ppo_epoch's checks, n_policies >= 1,
 * policy_stride at least b747_policy_num_params(obs_dim) and a multiple of 4, lr != NULL.  No kernel is batched over
 * members: 4 launches per member and minibatch. */
int32_t b747_ppo_epoch_population(float *theta /* [n_policies][policy_stride] */, int32_t n_policies,
                                  int64_t policy_stride, int32_t obs_dim, const float *obs, const float *act,
                                  const float *old_logp, const float *adv, const float *ret,
                                  const int64_t *perm /* [n_policies][n_rows] */, int64_t n_rows, int64_t batch_size,
                                  double clip_range, double ent_coef, double vf_coef, void *workspace,
                                  float *grad /* [P], reused */, float *m, float *v /* [n_policies][P] */,
                                  int64_t *t /* [n_policies] */, double max_grad_norm,
                                  const double *lr /* host, [n_policies] */, double beta1, double beta2, double eps,
                                  float *stats /* [n_policies][ceil(n_rows / batch_size)][8] */, void *stream);
/* b747_ppo_epoch_population with the kernels batched over members (additive under ABI 15): per minibatch
 * FOUR launches for a whole chunk of members -- member-batched siblings of the four update kernels, the member on
 * blockIdx.y, each running the single-member kernel's text on its member's pointers, with the grid x extent, the tile
 * assignment and every summation order of the member's own launch -- so theta, m, v, t and stats get the bits of
 * b747_ppo_epoch_population.  Differences in the arguments: no grad (each member's gradient vector lives in its slice
 * of the workspace); lr_dev is a DEVICE array [n_policies]; workspace_bytes says how much workspace there is.
 * b747_ppo_epoch_batched_workspace(obs_dim, batch_size): bytes PER MEMBER, 1024 + 72 n_wg + 4 P (n_wg + 1) rounded up
 * to a multiple of 16, with n_wg = min(256, ceil(ceil(batch_size / 32) / 2)) and P = 128 obs_dim + 8579 (2 x 64 fp64
 * advantage partials, 9 x n_wg fp64 row sums, n_wg partial gradient vectors, the gradient vector);
 * -hipErrorInvalidValue for an unsupported obs_dim or batch_size < 2.
 * Members are processed in chunks of min(n_policies, workspace_bytes / per member, 65535 -- a grid's y extent): a chunk
 * runs all its minibatches, then the next chunk starts.  Members are independent, so the chunking changes no bit; a
 * workspace for all members means the fewest launches.  workspace: 16-byte aligned, the caller's, its contents mean
 * nothing between calls.  Everything is validated before the first launch: b747_ppo_epoch_population's checks,
 * workspace_bytes at least one member's, lr_dev != NULL; -hipErrorInvalidValue with the argument named in
 * b747_last_error.  Stream-ordered, graph-capturable, allocates nothing, synchronises nothing, reads nothing back. */
int64_t b747_ppo_epoch_batched_workspace(int32_t obs_dim, int64_t batch_size);
int32_t b747_ppo_epoch_batched(float *theta /* [n_policies][policy_stride] */, int32_t n_policies, int64_t policy_stride,
                               int32_t obs_dim, const float *obs, const float *act, const float *old_logp,
                               const float *adv, const float *ret, const int64_t *perm /* [n_policies][n_rows] */,
                               int64_t n_rows, int64_t batch_size, double clip_range, double ent_coef, double vf_coef,
                               void *workspace, int64_t workspace_bytes, float *m, float *v /* [n_policies][P] */,
                               int64_t *t /* [n_policies] */, double max_grad_norm,
                               const double *lr_dev /* device, [n_policies] */, double beta1, double beta2, double eps,
                               float *stats /* [n_policies][ceil(n_rows / batch_size)][8] */, void *stream);

/* ---- per-member PPO hyper-parameters for a population (additive under ABI 15) ----
 * A hyper-parameter table is [n_policies][B747_PPO_HYPER_COLS] doubles, one 64-byte row per member, the columns named
 * below.  Every entry point that takes one takes this layout -- as a HOST table (hyper) or a DEVICE table (hyper_dev),
 * as its comment says -- and reads only its own columns; the reserved column is written 0 and never read.  What a
 * member cannot have of its own are the values that change shapes: n_steps, batch_size, the number of epochs and the
 * network's architecture stay the population's. */
#define B747_PPO_HYPER_COLS 8
#define B747_PPO_HYPER_LR 0             /* torch.optim.Adam's lr */
#define B747_PPO_HYPER_CLIP_RANGE 1
#define B747_PPO_HYPER_ENT_COEF 2
#define B747_PPO_HYPER_VF_COEF 3
#define B747_PPO_HYPER_MAX_GRAD_NORM 4
#define B747_PPO_HYPER_GAMMA 5
#define B747_PPO_HYPER_GAE_LAMBDA 6     /* (column 7: reserved; b747_a2c_update_population's B747_PPO_HYPER_OPTIMIZER) */
/* b747_ppo_epoch_population with member p's clip_range, ent_coef, vf_coef, max_grad_norm and lr taken from row p of
 * the HOST table hyper [n_policies][8] in place of the five arguments: the same host loop over the members of
 * b747_ppo_epoch's launches, each with its member's scalars as kernel arguments -- the bits of n_policies
 * b747_ppo_epoch calls with those scalars.  The table is read during the call only.  Validation:
 * b747_ppo_epoch_population's checks, and hyper != NULL (its values are the caller's to check: ppo.hyper_table). */
int32_t b747_ppo_epoch_population_hyper(float *theta /* [n_policies][policy_stride] */, int32_t n_policies,
                                        int64_t policy_stride, int32_t obs_dim, const float *obs, const float *act,
                                        const float *old_logp, const float *adv, const float *ret,
                                        const int64_t *perm /* [n_policies][n_rows] */, int64_t n_rows,
                                        int64_t batch_size, const double *hyper /* host, [n_policies][8] */,
                                        void *workspace, float *grad /* [P], reused */, float *m,
                                        float *v /* [n_policies][P] */, int64_t *t /* [n_policies] */, double beta1,
                                        double beta2, double eps,
                                        float *stats /* [n_policies][ceil(n_rows / batch_size)][8] */, void *stream);
/* b747_ppo_epoch_batched with the DEVICE table hyper_dev [n_policies][8] in place of clip_range, ent_coef, vf_coef,
 * max_grad_norm and lr_dev: the same chunks, grids and launch order, with siblings of three of its kernels (k_hyp_grad,
 * k_hyp_reduce, k_hyp_adam) that load member blockIdx.y's values from its table row -- workgroup-uniform loads -- before
 * they run the unchanged kernel text; ent_coef and vf_coef are rounded to float in the reduce kernel, as the host does
 * for b747_ppo_epoch_batched.  theta, m, v, t and stats get the bits of b747_ppo_epoch_population_hyper on the same
 * table.  The table is read when the kernels run: a row changed on the stream between two calls (or two replays of a
 * captured call) holds from the next one on.  Its values cannot be checked here.  workspace:
 * b747_ppo_epoch_batched_workspace's, unchanged.  Validation: b747_ppo_epoch_batched's checks with hyper_dev != NULL for
 * lr_dev's.  Stream-ordered, graph-capturable, allocates nothing, synchronises nothing, reads nothing back. */
int32_t b747_ppo_epoch_batched_hyper(float *theta /* [n_policies][policy_stride] */, int32_t n_policies,
                                     int64_t policy_stride, int32_t obs_dim, const float *obs, const float *act,
                                     const float *old_logp, const float *adv, const float *ret,
                                     const int64_t *perm /* [n_policies][n_rows] */, int64_t n_rows, int64_t batch_size,
                                     const double *hyper_dev /* device, [n_policies][8] */, void *workspace,
                                     int64_t workspace_bytes, float *m, float *v /* [n_policies][P] */,
                                     int64_t *t /* [n_policies] */, double beta1, double beta2, double eps,
                                     float *stats /* [n_policies][ceil(n_rows / batch_size)][8] */, void *stream);

/* ---- generalized advantage estimation in one launch (ABI 13; PPO.compute_gae, SB3 1.4
 * RolloutBuffer.compute_returns_and_advantage) ----
 * rew, val, adv, ret [T][N] float and done [T][N] bytes (0 / 1), time-major (row t * N + i); last_value [N]: the value
 * of the observation after the last step.  With g = (float)gamma and gl = (float)(gamma * gae_lambda) (the double
 * product rounded once), per env a = 0 and for t = T-1 .. 0:
 *   nv = t == T-1 ? last_value[i] : val[(t+1) N + i];   nt = done[t N + i] ? 0.f : 1.f;
 *   delta = (rew + ((g * nv) * nt)) - val;   a = delta + ((gl * nt) * a);   adv[t N + i] = a;   ret[t N + i] = a + val
 * -- one fp32 rounding per operation, in this order, with no FMA contraction: the operation sequence of the torch loop
 * in PPO.compute_gae, whose results it reproduces bit for bit.  One lane per env.  adv and ret must not overlap rew,
 * val, done or last_value (not detected).  A NULL pointer, T < 0 or N < 0 returns -hipErrorInvalidValue before
 * anything reaches the device (b747_last_error names the argument); T == 0 or N == 0 returns 0 and launches nothing.
 * Stream-ordered, graph-capturable, no allocation. */
int32_t b747_ppo_gae(const float *rew, const float *val, const uint8_t *done, const float *last_value,
                     int32_t T, int64_t N, double gamma, double gae_lambda, float *adv, float *ret, void *stream);
/* b747_ppo_gae for a population (additive under ABI 15): env i belongs to member i / envs_per_policy and
 * runs b747_ppo_gae's recurrence with g = (float)gamma and gl = (float)(gamma * gae_lambda) of that member's row of the
 * DEVICE table hyper_dev [n_policies][B747_PPO_HYPER_COLS] (columns B747_PPO_HYPER_GAMMA and _GAE_LAMBDA; the product
 * in fp64, rounded once, in the kernel: the host's rounding in b747_ppo_gae) -- the bits of one b747_ppo_gae call per
 * member on its own columns with its own scalars.  One lane per env, one launch; a workgroup is one wave, so its
 * member is uniform and the two doubles are loaded once.  The table is read when the kernel runs (see
 * b747_ppo_epoch_batched_hyper); its values cannot be checked here.  -hipErrorInvalidValue before anything reaches the
 * device (b747_last_error names the argument) for a NULL pointer, T < 0, N < 0, n_policies < 1, envs_per_policy not a
 * positive multiple of 64, or -- with N > 0 -- N outside ((n_policies - 1) * envs_per_policy, n_policies *
 * envs_per_policy] (the last member may be partial); T == 0 or N == 0 returns 0 and launches nothing.  Stream-ordered,
 * graph-capturable, no allocation. */
int32_t b747_ppo_gae_population(const float *rew, const float *val, const uint8_t *done, const float *last_value,
                                int32_t T, int64_t N, int32_t n_policies, int32_t envs_per_policy,
                                const double *hyper_dev /* device, [n_policies][8] */, float *adv, float *ret,
                                void *stream);

/* ---- the minibatch sample orders of a population, drawn on the device (additive under ABI 15; DESIGN.md 18;
 * PopulationPPO(sample_order="device")) ----
 * Row perm[p] receives a uniformly drawn order of member p's n_rows = T * envs_per_policy rollout rows, as the global
 * row numbers t * N + p * envs_per_policy + j that b747_ppo_epoch_population and its siblings read.  The order is fixed
 * by this definition, not by the kernel: local row l = t * envs_per_policy + j gets the 32-bit word u(p, l), word l & 3
 * of the Philox4x32-10 block (the rounds of the reset draws and the action noise) with
 *   sb  = step_base ? *step_base : 0                          (read on the device, when the kernel runs)
 *   K   = (seed ^ 0x6F72646572733A31) ^ ((sb >> 32) * 0x9E3779B97F4A7C15),   key (lo32(K), hi32(K))
 *   ctr = (l >> 2, p, lo32(sb), epoch)
 * and the rows are written in ascending order of the 64-bit key (u << 32) | l: a stable argsort of u, ties broken by l.
 * The tag in K keeps the stream apart from the action noise (key seed ^ (ctr >> 32) * C) and the reset draws.
 * b747_ppo_rollout_population advances *step_base, so a captured call replayed after every rollout draws fresh orders;
 * `epoch` tells an iteration's epochs apart.  One workgroup per member sorts the keys in LDS (bitonic, 8 bytes per key,
 * padded to a power of two): n_rows <= 16384 (128 KiB of the CU's 160) is the limit of this entry point.
 * -hipErrorInvalidValue before anything reaches the device (b747_last_error names the argument) for perm == NULL,
 * n_policies < 1, T < 0, envs_per_policy not a positive multiple of 64, n_policies * envs_per_policy > N, or
 * T * envs_per_policy > 16384; T == 0 returns 0 and launches nothing.  Stream-ordered, graph-capturable, allocates
 * nothing, synchronises nothing, reads nothing back. */
int32_t b747_ppo_sample_orders(int64_t *perm /* device, [n_policies][T * envs_per_policy] */, int32_t n_policies,
                               int32_t T, int32_t envs_per_policy, int64_t N, uint64_t seed,
                               const uint64_t *step_base /* device, nullable: 0 */, uint32_t epoch, void *stream);

/* ---- the reference's ControlTestCallback kept on the device (additive under ABI 15; DESIGN.md 19;
 * ppo.ControlTest) ----
 * One call books ONE step-test evaluation of a population -- what b747_eval_population / b747_eval_episodes left in
 * eval_out -- `repeat` times, as neural/callbacks.py:90-119 does per callback call.  Member p's reported envs are
 * p * envs_per_policy + [0, n_refs).  Per member, in float64:
 *   per env     settling_time, |overshoot| and quality = exp(-60 * 0.1 * itse / (tk * (vref * vref))), evaluated in
 *               that order (Controller.quality, core/controller.py:336)
 *   last[p]     the mean of each over the n_refs envs: (settling_time, overshoot, quality)
 *   repeat x    push last[p] into ring[.][p][count[p] % window], ++count[p]; window_mean[p] = the mean of the
 *               min(count[p], window) newest entries, oldest first; if window_mean[p].quality > best_quality[p] (strict:
 *               a NaN never saves) best_quality[p] = it, best_eval[p] = the index of this push (count[p] - 1), and the
 *               member is marked
 *   save        a marked member's row params[p] is copied to best_params[p] once, after the pushes (16-byte loads and
 *               stores by the whole workgroup; both rows 16-byte aligned); no other row is touched
 * Every mean is taken in the order of NumPy's np.mean of a list of n <= 128 values a: sequentially from 0 for n < 8;
 * otherwise r[j] = a[j] (j < 8), r[j] += a[i + j] for i = 8, 16, .. < n - n % 8, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
 * (r6 + r7)), the last n % 8 values added in order; divided by n.  Given the same last[p] the windows, the decisions
 * and the snapshots are therefore the callback's exactly; last[p].quality itself differs from NumPy's by the two
 * libraries' exp (about 1 ulp each).  More than 128 references are summed in the same eight-sum order (NumPy would
 * split the range there).
 * The state is the caller's, device memory, read and rewritten by every call: ring [3][n_members][window] (metric-major),
 * count [n_members] (pushes so far), last and window_mean [n_members][3], best_quality [n_members], best_eval
 * [n_members] (-1: nothing saved yet), best_params [n_members][stride].  A fresh tracker has count 0, best_quality 0 and
 * best_eval -1; ring, last and window_mean need no initial value.
 * One workgroup per member; one lane per metric keeps the books in an LDS copy of the member's windows.  No atomics:
 * the same inputs give the same bits.  -hipErrorInvalidValue before anything reaches the device (b747_last_error names
 * the argument) for a NULL pointer, n_members < 1, envs_per_policy not a positive multiple of 64, n_refs outside
 * [1, envs_per_policy], n_eval outside ((n_members - 1) * envs_per_policy + n_refs - 1, n_members * envs_per_policy],
 * window outside [1, 128], repeat outside [1, 256], stride < 4 or not a multiple of 4, or tk not above 0.
 * Stream-ordered, graph-capturable, allocates nothing, synchronises nothing, reads nothing back. */
int32_t b747_ppo_track_best(const double *eval_out /* device, [B747_NEVAL][n_eval] */, int64_t n_eval,
                            const double *vref /* device, [n_eval], rad */, double tk, int32_t n_members,
                            int32_t envs_per_policy, int32_t n_refs, int32_t window, int32_t repeat,
                            const float *params /* device, [n_members][stride] */, int64_t stride,
                            double *ring /* device, [3][n_members][window] */, int64_t *count, double *last,
                            double *window_mean, double *best_quality, int64_t *best_eval,
                            float *best_params /* device, [n_members][stride] */, void *stream);

/* ---- one A2C update on the device (additive under ABI 15; ppo.A2C; SB3 1.4 A2C.train) ----
 * For the policy of b747_ppo_grad (the same theta, the same obs_dims) ONE gradient step over the rows r = idx[0 .. batch)
 * of the time-major rollout buffers -- idx may be NULL: the rows 0 .. batch - 1, A2C's whole buffer -- of the loss
 *   mean(-A logp) + ent_coef (-entropy) + vf_coef mean((ret - value)^2)
 * with A = adv, or with normalize_advantage != 0 A = (adv - mean) / (std + 1e-8) over the batch (unbiased std, fp64 sums:
 * b747_ppo_grad's statistics; without it that launch is skipped).  Two calls, so that a data-parallel all-reduce of the
 * flat gradient fits between them, or b747_a2c_update for both; all stream-ordered and graph-capturable, no allocation,
 * no synchronisation, no floating-point atomics: the same inputs give the same bits.  All pointers are device memory.
 *
 * b747_a2c_grad: grad [P] = the loss's gradient (flat_params order); stats [8] = the policy loss mean(-A logp), the
 * value loss, the entropy loss, 0, 0, mean |A logp| (the magnitude of the terms the policy loss sums), 0, and the loss.
 * b747_ppo_grad's arithmetic (fp64 forward, fp32 matrix-core backward products, the gradients of action_net.bias,
 * value_net.bias and log_std summed in fp64), grid and workspace (b747_ppo_update_workspace(obs_dim) bytes).  batch >= 1;
 * >= 2 with normalize_advantage.
 * b747_ppo_rmsprop: g = grad_scale grad; coef = min(1, max_grad_norm / (|g|_2 + 1e-6)) (torch clip_grad_norm_); gc = g
 * coef; sq = alpha sq + (1 - alpha) gc^2; theta -= lr gc / (sqrt(sq) + eps) (tf_like == 0: torch.optim.RMSprop, not
 * centred, momentum 0, no weight decay; sq starts at zeros) or theta -= lr gc / sqrt(sq + eps) (tf_like != 0: SB3's
 * RMSpropTFLike; sq starts at ONES, which the caller fills); *t += 1 (one device int64, as b747_ppo_adam's).  theta, sq
 * [n_params]; element arithmetic in fp64, stored as fp32; grad is not modified.
 * b747_a2c_update: the launches of b747_a2c_grad, then those of the optimiser with grad_scale 1 and n_params = P, from
 * one host call -- the same kernels, arguments and order, the same bits.  optimizer B747_OPT_RMSPROP / _RMSPROP_TF:
 * b747_ppo_rmsprop on state0 = sq (state1 is not read and may be NULL) with alpha and eps.  B747_OPT_ADAM: b747_ppo_adam
 * on state0 = m, state1 = v with betas 0.9 / 0.999 and eps (SB3's use_rms_prop=False; alpha is not read).
 * All return -hipErrorInvalidValue, before anything reaches the device (b747_last_error names the argument), for a
 * NULL pointer other than idx (and state1 where it is not read), an obs_dim without kernels, batch < 1 (< 2 with
 * normalize_advantage), n_params < 1, an lr, eps or max_grad_norm that is not finite and above 0, alpha outside [0, 1)
 * or an unknown optimizer. */
#define B747_OPT_ADAM 0
#define B747_OPT_RMSPROP 1
#define B747_OPT_RMSPROP_TF 2
int32_t b747_a2c_grad(const float *theta, int32_t obs_dim, const float *obs, const float *act, const float *adv,
                      const float *ret, const int64_t *idx /* may be NULL */, int64_t batch, int32_t normalize_advantage,
                      double ent_coef, double vf_coef, void *workspace, float *grad, float *stats, void *stream);
int32_t b747_ppo_rmsprop(float *theta, float *sq, int64_t *t, const float *grad, int64_t n_params, double grad_scale,
                         double max_grad_norm, double lr, double alpha, double eps, int32_t tf_like, void *stream);
int32_t b747_a2c_update(float *theta, int32_t obs_dim, const float *obs, const float *act, const float *adv,
                        const float *ret, const int64_t *idx /* may be NULL */, int64_t batch,
                        int32_t normalize_advantage, double ent_coef, double vf_coef, void *workspace, float *grad,
                        float *stats, int32_t optimizer, float *state0, float *state1 /* Adam's v, else may be NULL */,
                        int64_t *t, double max_grad_norm, double lr, double alpha, double eps, void *stream);

/* ---- one A2C update of every member of a population (additive under ABI 15; ppo.PopulationA2C) ----
 * b747_a2c_update for n_policies members at once: member p = blockIdx.y of member-batched siblings of its kernels
 * (k_apop_adv_stats, k_apop_grad, k_apop_reduce, k_apop_opt) -- about four launches for the whole population in place
 * of four per member.  Member p's parameters are theta + p * policy_stride; its minibatch is the rows
 * rows[p * rows_stride + (0 .. batch)) of the time-major rollout buffers (an index table, device int64,
 * [n_policies][rows_stride]: a member's rows t * N + p * envs_per_member + i are not a range; a prefix of a table row
 * serves a shorter rollout, hence rows_stride >= batch); its ent_coef, vf_coef, max_grad_norm, lr and optimiser are
 * columns B747_PPO_HYPER_ENT_COEF, _VF_COEF, _MAX_GRAD_NORM, _LR and _OPTIMIZER of row p of the DEVICE table hyper_dev
 * [n_policies][B747_PPO_HYPER_COLS], read when the kernels run (see b747_ppo_epoch_batched_hyper; its values cannot be
 * checked here); B747_PPO_HYPER_CLIP_RANGE, _GAMMA and _GAE_LAMBDA are not read.  Column B747_PPO_HYPER_OPTIMIZER holds
 * a B747_OPT_* value as a double: 1 (B747_OPT_RMSPROP) and 2 (B747_OPT_RMSPROP_TF) run b747_ppo_rmsprop's arithmetic
 * on state0[p] = sq with rms_alpha and rms_eps (a TF-like member's row starts at ONES, the caller's fill); ANY OTHER
 * VALUE means Adam: b747_ppo_adam's arithmetic on state0[p] = m and state1[p] = v with adam_beta1, adam_beta2 and
 * adam_eps.  Every kind adds 1 to t[p].  state0 and state1 are [n_policies][P] (P = the policy's parameter count; both
 * required, whatever the members' optimisers), t [n_policies], stats [n_policies][8] in b747_a2c_grad's layout.
 * normalize_advantage, the optimisers' alpha, betas and eps values are shared.  The PPO entry points keep ignoring
 * column 7.
 * workspace: one slice of b747_ppo_epoch_batched_workspace(obs_dim, batch) bytes per member (batch 1 takes batch 2's
 * size); with fewer, the members run in chunks of min(n_policies, workspace_bytes / slice, 65535), which changes no bit.
 * theta, state0, state1, t and stats get the bits of n_policies b747_a2c_update calls with idx = the member's table row
 * and the member's scalars and optimiser.  -hipErrorInvalidValue before anything reaches the device (b747_last_error
 * names the argument and this entry point) for a NULL pointer, an obs_dim without kernels, n_policies < 1, a
 * policy_stride below the parameter count or not a multiple of 4, batch < 1 (< 2 with normalize_advantage),
 * rows_stride < batch, workspace_bytes below one slice, rms_alpha, adam_beta1 or adam_beta2 outside [0, 1), or an eps
 * that is not finite and above 0.  Stream-ordered, graph-capturable, allocates nothing, synchronises nothing, reads no
 * per-member value on the host. */
#define B747_PPO_HYPER_OPTIMIZER 7
int32_t b747_a2c_update_population(float *theta /* [n_policies][policy_stride] */, int32_t n_policies,
                                   int64_t policy_stride, int32_t obs_dim, const float *obs, const float *act,
                                   const float *adv, const float *ret,
                                   const int64_t *rows /* device, [n_policies][rows_stride] */, int64_t rows_stride,
                                   int64_t batch, int32_t normalize_advantage,
                                   const double *hyper_dev /* device, [n_policies][8] */, void *workspace,
                                   int64_t workspace_bytes, float *state0, float *state1 /* [n_policies][P] */,
                                   int64_t *t /* [n_policies] */, double rms_alpha, double rms_eps, double adam_beta1,
                                   double adam_beta2, double adam_eps, float *stats /* [n_policies][8] */,
                                   void *stream);

/* ---- exploit and explore for a population, on the device (additive under ABI 15; DESIGN.md 22;
 * PopulationPPO.exploit, ppo.PBT) ----
 * The step of a truncation-selection population-based schedule (Jaderberg et al., 2017): the n_replace worst members
 * by `score` are each re-seeded from one of the n_replace best, drawn at random, and take its parameters, optimiser
 * state and -- perturbed -- its row of the hyper-parameter table.  Decided and done on the device; nothing is read back.
 * All pointers are device memory except `explore`.
 *
 * Order.  s'(p) = score[p], a NaN read as -inf.  Member q is BETTER than p when s'(q) > s'(p), or s'(q) == s'(p) and
 * q < p (IEEE comparisons: -0.0 == +0.0).  rank(p) = the number of members better than p: a total order, every rank
 * 0 .. n_members - 1 taken once.  WINNERS have rank < n_replace, LOSERS rank >= n_members - n_replace;
 * n_replace <= n_members / 2 keeps the two sets disjoint, so a source row is never written and the step runs in place.
 *
 * Draw.  Loser p takes ONE Philox4x32-10 block (the rounds of the reset draws, the action noise and
 * b747_ppo_sample_orders) with
 *   sb  = step_base ? *step_base : 0                          (read on the device, when the kernel runs)
 *   K   = (seed ^ 0x6578706C6F697431) ^ ((sb >> 32) * 0x9E3779B97F4A7C15),   key (lo32(K), hi32(K))
 *   ctr = (p, 0, lo32(sb), round)
 * The tag ("exploit1") keeps the stream apart from the action noise and the sample orders; `round` tells the exploit
 * steps of one step_base apart.  Word 0 picks the source: q = the winner of rank w = (uint64(word0) * n_replace) >> 32.
 * Bit j of word 1 picks column j's factor: 0 gives f_lo, 1 gives f_hi.
 *
 * Decision.  Loser p with source q is REPLACED only if s'(q) > s'(p), strictly: a population of equal or all-NaN
 * scores changes nothing, and a NaN member is never a source.  src_of[p] = q where p is replaced and src_of[p] = p for
 * every other member (winners, the middle, losers that were not replaced); all n_members entries are written by every
 * call.
 *
 * A replaced member p receives from q:
 *   params[p][0 .. stride)           the whole stride, so the packed sections travel (16-byte loads and stores; rows
 *                                    16-byte aligned)
 *   state0[p], state1[p]             [0 .. n_state) each (4-byte elements: n_state is odd for the product's policies,
 *                                    so the rows of two members differ in 16-byte phase; no alignment is assumed)
 *   upd_t[p]
 *   rew[p][0 .. 8)                   if rew is given ([n_members][8] doubles: b747_ppo_rollout_population's rew_pop)
 *   hyper[p][0 .. 8)                 if hyper is given ([n_members][B747_PPO_HYPER_COLS]).  Without `explore` an exact
 *                                    copy.  With it, in float64, column j becomes
 *                                      fmin(fmax(hyper[q][j] * f, min_j), max_j),   explore[j] = (f_lo, f_hi, min, max)
 *                                    -- one multiply (not contracted), two selects; C's fmax / fmin: a NaN product
 *                                    gives min_j.  A column with factors 1 and bounds -inf / +inf is an exact copy
 *                                    (b747_a2c_update_population's optimiser column is passed as such a column).
 * No row of any other member is touched, in any buffer.
 *
 * explore is a HOST array [B747_PPO_HYPER_COLS][4], read and validated before the call returns (as
 * b747_ppo_epoch_population's learning rates) and passed to the kernel by value: a capture holds a fixed exploration
 * rule.  step_base may be NULL (0).  hyper may be NULL; then explore must be NULL too.  explore may be NULL with a
 * table: rows then travel unchanged.  rew may be NULL.
 *
 * -hipErrorInvalidValue before anything reaches the device (b747_last_error names this entry point and the argument)
 * for a NULL score, params, state0, state1, upd_t or src_of; n_members outside [2, 4096] (one workgroup ranks the
 * members: 8 bytes of score and two 16-bit tables each in static LDS); n_replace outside [1, n_members / 2]; stride < 4
 * or not a multiple of 4; n_state < 1; explore without hyper; an explore row with a factor that is not finite and above
 * 0, f_lo > f_hi, a NaN bound, or min > max.
 * Two launches (k_exploit_plan: one workgroup; k_exploit_copy: a grid of (chunks, n_members) workgroups, those of a
 * member that is not replaced returning at once).  Stream-ordered, graph-capturable, allocates nothing, synchronises
 * nothing, reads nothing back, no atomics: the same inputs give the same bits. */
int32_t b747_ppo_exploit(const double *score /* device, [n_members] */, int32_t n_members, int32_t n_replace,
                         uint64_t seed, const uint64_t *step_base /* device, nullable: 0 */, uint32_t round,
                         float *params /* device, [n_members][stride] */, int64_t stride,
                         float *state0, float *state1 /* device, [n_members][n_state] */, int64_t n_state,
                         int64_t *upd_t /* device, [n_members] */, double *hyper /* device, [n_members][8], nullable */,
                         const double *explore /* HOST, [8][4], nullable */,
                         double *rew /* device, [n_members][8], nullable */, int32_t *src_of /* device, [n_members] */,
                         void *stream);

/* Human-readable text of the last error returned on this thread. */
const char *b747_last_error(void);

#ifdef __cplusplus
}
#endif
