// b747_fast.hip -- the FAST variant's kernels (b747_lanes.h instantiated with FAST = true).
// A separate translation unit so that FMA contraction applies to FAST only: the FAITHFUL
// kernels in b747_kernels.hip keep the DLL's separate mul/add roundings (-ffp-contract=off),
// while here every a*b+c of the dynamics becomes one v_fma_f64 (one rounding instead of two:
// within FAST's per-step tolerance).
#pragma clang fp contract(fast)

#include "b747_lanes.h"
#include "b747_split.h"
#include "b747_model_split.h"


#define B747_POLICY_NO_KERNELS   // the policy kernels live in b747_kernels.hip; this unit reuses actor_critic
#include "b747_policy.h"
#include "b747_ppo_split.h"

namespace b747 {

static_assert(kSplitEnvs == kLargeWgEnvs && kBlock == kLargeWgEnvs && kMsEnvs == kSmallWgEnvs,
              "the plans' workgroup sizes (b747_dispatch.h) are the kernels' defaults");

bool launch_env_steps_fast(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C, const EnvPlan &p,
                           const float *actions, int32_t n_env_steps, float *obs_seq, float *reward_seq,
                           uint8_t *done_seq, hipStream_t s)
{
    // the training configuration: each env over a flight (and an ahead) and a control wave.  MIX: the same kernels with
    // the flight aerodynamics in fp32 (include/b747.h B747_VARIANT_MIXED).  256 envs per workgroup (the waves of an env
    // on one SIMD), or 64 (one wave per role, each on a SIMD of its own): plan_env, b747_dispatch.h
    const bool small = p.envs_per_wg == kSmallWgEnvs;
    if (p.kernel == EnvKernel::STEP_SPLIT) {   // the per-step API (b747_split.h)
        with_bools([&](auto x64, auto mix, auto sm) {
            constexpr int E = decltype(sm)::value ? kSmallWgEnvs : kSplitEnvs;
            hipLaunchKernelGGL((k_env_step_split<storage_t<decltype(x64)>, decltype(mix)::value, E>), dim3(grid_for(b.n, E)),
                               dim3(3 * E), 0, s, b.n, (const void *)b.X, (const double *)b.aero_err, (const uint32_t *)b.k,
                               (const double *)b.disc, (const uint8_t *)b.flags, actions, b, cfg, obs_seq, reward_seq,
                               done_seq);
        }, p.x_f64, p.mix, small);
        return true;
    }
    if (p.kernel == EnvKernel::ROLLOUT_SPLIT) {
        // K steps per launch (b747_env_rollout), or one env step of n_sub > 1 DLL steps: the rollout kernel of
        // b747_ppo_rollout without the policy -- the two roles hand off per wave pair and the flight wave never waits
        // for the next step's controller (b747_ppo_split.h)
        const RolloutArgs ra{nullptr, 0, nullptr, actions, n_env_steps, obs_seq, nullptr, nullptr, reward_seq, done_seq,
                             0.0f, 0.0f, nullptr};
        with_bools([&](auto x64, auto sub, auto mix, auto sm) {
            constexpr int E = decltype(sm)::value ? kSmallWgEnvs : kSplitEnvs;
            hipLaunchKernelGGL((k_rollout_split<false, storage_t<decltype(x64)>, decltype(sub)::value, decltype(mix)::value, E>),
                               dim3(grid_for(b.n, E)), dim3(2 * E), 0, s, b, cfg, ra);
        }, p.x_f64, p.sub, p.mix, small);
        return true;
    }
    return launch_env_steps<true>(b, cfg, C, p, actions, n_env_steps, obs_seq, reward_seq, done_seq, s);
}

bool launch_model_step_fast(const b747_model_batch &b, const Consts &C, const ModelPlan &p, int32_t n_steps, hipStream_t s)
{
    // the DLL's default constants: each env over three waves (b747_model_split.h) -- one step (BASELINE config 2's
    // per-step calls), or K steps with the state in registers for small batches (config 2's 100-step launches)
    const dim3 g(grid_for(b.n, kMsEnvs)), blk(kMsBlock);
    if (p.kernel == ModelKernel::STEP_SPLIT) {
        with_bools([&](auto x64) { hipLaunchKernelGGL((k_model_step_split<storage_t<decltype(x64)>>), g, blk, 0, s, b); },
                   p.x_f64);
        return true;
    }
    if (p.kernel == ModelKernel::STEPS_SPLIT) {
        with_bools([&](auto x64) { hipLaunchKernelGGL((k_model_steps_split<storage_t<decltype(x64)>>), g, blk, 0, s, b, n_steps); },
                   p.x_f64);
        return true;
    }
    return launch_model_step<true>(b, C, p, n_steps, s);
}

void launch_ppo_rollout_fast(const b747_env_batch &b, const b747_env_config &cfg, const float *params, uint64_t seed,
                             const uint64_t *step_base, int32_t T, float *obs_buf, float *act_buf, float *logp_buf,
                             float *val_buf, float *rew_buf, uint8_t *done_buf, float act_lo, float act_hi,
                             hipStream_t s)
{
    const RolloutArgs ra{params, seed, step_base, nullptr, T, obs_buf, act_buf, logp_buf, rew_buf, done_buf, act_lo, act_hi,
                         val_buf};
    // sub: sample_time > dt (main.py's 0.05), n_sub DLL steps per env step (core/controller.py:258-264); 64 envs per
    // workgroup: one flight / control pair, as b747_env_rollout
    const PpoPlan p = plan_ppo_rollout(b, cfg);
    with_bools([&](auto sub, auto mix, auto sm) {
        constexpr int E = decltype(sm)::value ? kSmallWgEnvs : kSplitEnvs;
        hipLaunchKernelGGL((k_rollout_split<true, double, decltype(sub)::value, decltype(mix)::value, E>), dim3(grid_for(b.n, E)),
                           dim3(2 * E), 0, s, b, cfg, ra);
    }, p.sub, p.mix, p.envs_per_wg == kSmallWgEnvs);
}

}  // namespace b747

#ifdef B747_STAMPS
// diagnostic build only: copy the per-wave phase stamps of the last FAST env-step launch to the host
extern "C" __attribute__((visibility("default"))) int b747_debug_stamps(unsigned long long *out, int n)
{
    const size_t bytes = sizeof(unsigned long long) * (size_t)(n < kStampWaves * kStampSlots ? n : kStampWaves * kStampSlots);
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_b747_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
#endif
