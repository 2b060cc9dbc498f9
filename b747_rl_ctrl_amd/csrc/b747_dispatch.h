/* b747_dispatch.h -- which kernel a call launches, and with what workgroup geometry: decided here, once, in host code
 * that includes no HIP header (tests/test_dispatch_plan.py compiles it with g++: tests/native/dispatch_check.cpp).
 * The entry points of b747_kernels.hip make a plan and hand it to the launchers (b747_lanes.h, b747_fast.hip), which
 * only turn it into template arguments; b747_env_kernel reports the same plan's kernel.  DESIGN.md 4 has the table. */
#pragma once

#include <stdint.h>

#include <type_traits>

#include "../../include/b747.h"
#include "b747_dynamics.h"
#include "b747_env.h"

namespace b747 {

/* ---- workgroup-geometry thresholds: the multi-wave kernels take 64 envs per workgroup (one wave per role, each role
 * on a SIMD of its own, n / 64 CUs at work instead of n / 256) up to the batch size where that stops paying ---- */
/* k_env_step_split: faster up to 32,768 envs, slower at 65,536 (profiles/r06/small_batch_env_step.txt) */
constexpr int64_t kStepSplitSmallMax = 32768;
/* k_rollout_split<false>: faster up to 16,384 envs, slower from 24,576 (profiles/r06/small_batch_env_step.txt) */
constexpr int64_t kRolloutSplitSmallMax = 16384;
/* k_rollout_split<true>: the policy then fits without spilling; faster up to 32,768 envs, slower at 65,536
 * (profiles/r06/small_batch_env_step.txt) */
constexpr int64_t kPpoRolloutSmallMax = 32768;
/* k_model_steps_split: three waves per env with the state in registers up to 16,384 envs; above, the one-wave kernel,
 * whose single wave per env keeps every SIMD at one wave per 64 envs (profiles/r06/config2_geometry.txt) */
constexpr int64_t kModelStepsSplitMax = 16384;
/* k_model_step: one wave per workgroup up to 16,384 envs, so that the waves spread over n / 64 CUs instead of sharing
 * n / 256 -- 9.36 against 10.25 us per one-step launch at 4,096 envs, 5.30 against 5.38 us per step at 100 steps a
 * launch (profiles/r06/config2_geometry.txt) */
constexpr int64_t kModelStepSmallMax = 16384;

constexpr int kSmallWgEnvs = 64, kLargeWgEnvs = 256;

/* The DLL's default constants (bitwise): such batches run the kernels specialised on them. */
inline bool is_default(const b747_consts &c)
{
    const Consts &d = kDefaultConsts;
    bool same = c.Iz == d.Iz && c.P == d.P && c.S == d.S && c.c_ == d.c_ && c.g == d.g && c.m0 == d.m0;
    for (int j = 0; j < 4; ++j) same = same && c.PID_CS[j] == d.PID_CS[j] && c.PID_SS[j] == d.PID_SS[j];
    return same;
}

/* ------------------------------------------------------------------ env step / rollout ---- */
enum class EnvKernel : int32_t { GENERIC = 0, DEFC = 1, RECORDING = 2, SPEC_ONE_WAVE = 3, STEP_SPLIT = 4, ROLLOUT_SPLIT = 5 };
static_assert((int)EnvKernel::GENERIC == B747_KERNEL_GENERIC && (int)EnvKernel::DEFC == B747_KERNEL_DEFC &&
                  (int)EnvKernel::RECORDING == B747_KERNEL_RECORDING &&
                  (int)EnvKernel::SPEC_ONE_WAVE == B747_KERNEL_SPEC_ONE_WAVE &&
                  (int)EnvKernel::STEP_SPLIT == B747_KERNEL_STEP_SPLIT &&
                  (int)EnvKernel::ROLLOUT_SPLIT == B747_KERNEL_ROLLOUT_SPLIT,
              "EnvKernel is the public B747_KERNEL_* code (b747_env_kernel returns it)");

struct EnvPlan {
    EnvKernel kernel;
    bool x_f64;
    bool mix;          /* the split kernels' fp32 flight aerodynamics (B747_VARIANT_MIXED); the one-wave kernels have none */
    bool sub;          /* ROLLOUT_SPLIT: n_sub > 1 DLL steps per env step */
    bool k1;           /* one env step of one DLL step (n_env_steps == 1 && n_sub == 1) */
    int envs_per_wg;   /* 64 or 256 */
};

/* spec: b747_set_specialization's setting (0 generic, 1 the split kernels, 2 the specialised one-wave kernel) */
inline EnvPlan plan_env(const b747_env_batch &b, const b747_env_config &cfg, bool default_consts, int spec,
                        int32_t n_env_steps)
{
    EnvPlan p{EnvKernel::DEFC, b.x_f64 != 0, false, false, n_env_steps == 1 && cfg.n_sub == 1, kLargeWgEnvs};
    if (b.sig) p.kernel = EnvKernel::RECORDING;
    else if (!default_consts) p.kernel = EnvKernel::GENERIC;
    else if (spec != 0 && spec_config_matches(cfg) && b.variant != B747_VARIANT_FAITHFUL)   /* FAITHFUL: DEFC */
        p.kernel = spec == 2 ? EnvKernel::SPEC_ONE_WAVE : (p.k1 ? EnvKernel::STEP_SPLIT : EnvKernel::ROLLOUT_SPLIT);
    if (p.kernel == EnvKernel::STEP_SPLIT || p.kernel == EnvKernel::ROLLOUT_SPLIT) {
        const bool step = p.kernel == EnvKernel::STEP_SPLIT;
        p.mix = b.variant == B747_VARIANT_MIXED;   /* (outside the split kernels MIXED runs the FAST one-wave kernels) */
        p.sub = !step && cfg.n_sub > 1;
        p.envs_per_wg = b.n <= (step ? kStepSplitSmallMax : kRolloutSplitSmallMax) ? kSmallWgEnvs : kLargeWgEnvs;
    }
    return p;
}

/* ------------------------------------------------------------------------ PPO rollout ---- */
/* b747_ppo_rollout's fused kernel covers the training configuration only, whatever b747_set_specialization says */
inline bool ppo_rollout_covers(const b747_env_batch &b, const b747_env_config &cfg, bool default_consts)
{
    return default_consts && spec_config_matches(cfg) && b.x_f64 && b.variant != B747_VARIANT_FAITHFUL &&
           b.obs_dim == 3 && b.n % 64 == 0 && !b.sig;
}

struct PpoPlan {
    bool mix, sub;
    int envs_per_wg;
};

inline PpoPlan plan_ppo_rollout(const b747_env_batch &b, const b747_env_config &cfg)
{
    return PpoPlan{b.variant == B747_VARIANT_MIXED, cfg.n_sub > 1,
                   b.n <= kPpoRolloutSmallMax ? kSmallWgEnvs : kLargeWgEnvs};
}

/* b747_ppo_rollout_lanes' one-wave kernel (k_rollout_lanes, b747_rollout_lanes.h) runs the generic lane code: every
 * configuration, constants, variant (MIXED as FAST) and n >= 1 that b747_env_step covers.  What it does not cover, as
 * the reason the entry point reports; NULL = covered. */
inline const char *ppo_rollout_lanes_refusal(const b747_env_batch &b)
{
    if (b.obs_dim != 3 && b.obs_dim != 5)
        return "b747_ppo_rollout_lanes: obs_dim (the one-wave rollout kernel runs a policy with PID_LIKE 3 or SPEED_MODE "
               "5 only; use b747_policy_act + b747_env_step)";
    if (!b.x_f64) return "b747_ppo_rollout_lanes: x_f64 (the one-wave rollout kernel keeps fp64 state only)";
    if (b.sig) return "b747_ppo_rollout_lanes: sig (no per-DLL-step signal recording inside the rollout kernel)";
    return nullptr;
}
inline bool ppo_rollout_lanes_covers(const b747_env_batch &b) { return ppo_rollout_lanes_refusal(b) == nullptr; }

/* ------------------------------------------------------------------------- model step ---- */
enum class ModelKernel : int32_t {
    ONE_WAVE = 0,      /* k_model_step: one wave per env, run-time constants */
    STEP_SPLIT = 1,    /* k_model_step_split: one step, three waves per env */
    STEPS_SPLIT = 2,   /* k_model_steps_split: K steps with the state in registers, three waves per env */
};

struct ModelPlan {
    ModelKernel kernel;
    bool x_f64;
    int envs_per_wg;   /* 64 or 256 (the three-wave kernels: always 64) */
};

/* The three-wave kernels take the DLL's default constants as literals, so they need them and the specialised kernels
 * switched on (spec != 0: 2 counts as 1, include/b747.h); FAITHFUL has the one-wave kernel only. */
inline ModelPlan plan_model(const b747_model_batch &b, bool default_consts, int spec, int32_t n_steps)
{
    const bool split = b.variant != B747_VARIANT_FAITHFUL && spec != 0 && default_consts;
    if (split && n_steps == 1) return ModelPlan{ModelKernel::STEP_SPLIT, b.x_f64 != 0, kSmallWgEnvs};
    if (split && b.n <= kModelStepsSplitMax) return ModelPlan{ModelKernel::STEPS_SPLIT, b.x_f64 != 0, kSmallWgEnvs};
    return ModelPlan{ModelKernel::ONE_WAVE, b.x_f64 != 0, b.n <= kModelStepSmallMax ? kSmallWgEnvs : kLargeWgEnvs};
}

/* --------------------------------------------- run-time bools to template arguments ---- */
/* with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): every combination of
 * f is instantiated, one is run.  storage_t turns the x_f64 one into the state's storage type. */
template <class F>
decltype(auto) with_bools(F &&f)
{
    return f();
}
template <class F, class... Rest>
decltype(auto) with_bools(F &&f, bool b0, Rest... rest)
{
    if (b0) return with_bools([&](auto... t) -> decltype(auto) { return f(std::true_type{}, t...); }, rest...);
    return with_bools([&](auto... t) -> decltype(auto) { return f(std::false_type{}, t...); }, rest...);
}
template <class X64>
using storage_t = std::conditional_t<X64::value, double, float>;

}  // namespace b747
