// b747_rollout_lanes.h -- a whole stochastic PPO rollout in one launch for every env configuration
// (b747_ppo_rollout_lanes, include/b747.h).
//
// b747_ppo_rollout's two-wave kernel (k_rollout_split<true>, b747_ppo_split.h) is specialised on one configuration.
// k_rollout_lanes is the general one: T steps of SB3's collect_rollouts for 64 envs per wave -- the policy
// (actor_critic<OD>), the Gaussian sample of k_policy_act (policy_noise, the same Philox counters), the
// generic lane code of b747_lanes.h for the env step (every control type / mode, reward, limiter setting and n_sub
// that k_env_steps covers; run-time constants), the rollout rows, and k_env_steps' episode end and auto-reset -- with
// the env state and the observation in registers across the steps.  It is k_eval_episodes (b747_eval.h) with noise,
// rows and resets instead of the step-response score, and keeps that kernel's shape: one wave per workgroup, no
// hand-off between waves, one loop bounded by T.  Instantiated by two translation units of its own,
// b747_rollout_lanes_faithful.hip and b747_rollout_lanes_fast.hip (as the evaluation kernel and for its reason: new
// kernels inside an existing unit changed the code generated for the kernels already there).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/b747.h"
#include "b747_dynamics.h"

namespace b747 {

// Where the value head runs.  obs_dim 3: not in the kernel at all -- the entry point launches k_policy_value<3> over
// the stored rows afterwards (b747_ppo_rollout's deferred pass, which also advances the counter): the batched pass
// costs less than the head does inside the latency-bound step loop (2.14 against 2.31 ms at 4,096 x 64,
// 63.7 against 69.1 ms at 4 x 2,048, within the spread at 65,536 x 64), and gives k_policy_act's bits.  obs_dim 5 has no
// batched value kernel (k_policy_value needs the matrix-core layer 1): in the step loop.
// -DB747_LANES_VALUE_IN_LOOP (diagnostic A/B build only, tools/exp_ppo_rollout_lanes.py --variants): in the loop for both.
#ifdef B747_LANES_VALUE_IN_LOOP
constexpr bool kLanesDeferValue3 = false;
#else
constexpr bool kLanesDeferValue3 = true;
#endif

struct RolloutLanesArgs {
    const float *params;          // packed policy (b747_policy_pack)
    uint64_t seed;
    const uint64_t *step_base;    // nullable = 0; read once per wave, advanced by the launch after this kernel
    int32_t T;
    float act_lo, act_hi;
    float *obs_buf, *act_buf, *logp_buf, *val_buf, *rew_buf;   // row t * n + i ([T][N][obs_dim] for obs_buf)
    uint8_t *done_buf;
};

// Defined in b747_rollout_lanes_fast.hip / b747_rollout_lanes_faithful.hip (hidden: not part of the C ABI); od = the
// policy's obs_dim (3 or 5).  advance (nullable): the counter to add T to, in a one-thread launch after the rollout
// (NULL where the deferred value pass advances it).
__attribute__((visibility("hidden"))) void launch_rollout_lanes_fast(const b747_env_batch &b, const b747_env_config &cfg,
                                                                     const Consts &C, const RolloutLanesArgs &ra, int od,
                                                                     uint64_t *advance, hipStream_t s);
__attribute__((visibility("hidden"))) void launch_rollout_lanes_faithful(const b747_env_batch &b,
                                                                         const b747_env_config &cfg, const Consts &C,
                                                                         const RolloutLanesArgs &ra, int od,
                                                                         uint64_t *advance, hipStream_t s);

// What the population form adds (b747_ppo_rollout_population; k_rollout_population, b747_rollout_population.h)
struct RolloutPopArgs {
    int64_t policy_stride;      // floats from one packed policy to the next
    int32_t waves_per_policy;   // envs_per_policy / 64: workgroup w flies policy (and reward row) w / waves_per_policy
    const double *rew_pop;      // [n_policies][8] reward constants in cfg->rew order, NULL = cfg->rew for every group
    float *last_val;            // [N] the value head on the observation the rollout ends on, nullable
};

// Defined in b747_rollout_population_fast.hip / b747_rollout_population_faithful.hip (hidden); advance (nullable):
// the counter to add T to, in a one-thread launch after the rollout
__attribute__((visibility("hidden"))) void launch_rollout_population_fast(const b747_env_batch &b,
                                                                          const b747_env_config &cfg, const Consts &C,
                                                                          const RolloutLanesArgs &ra,
                                                                          const RolloutPopArgs &pa, int od,
                                                                          uint64_t *advance, hipStream_t s);
__attribute__((visibility("hidden"))) void launch_rollout_population_faithful(const b747_env_batch &b,
                                                                              const b747_env_config &cfg, const Consts &C,
                                                                              const RolloutLanesArgs &ra,
                                                                              const RolloutPopArgs &pa, int od,
                                                                              uint64_t *advance, hipStream_t s);
}  // namespace b747

#ifndef B747_ROLLOUT_LANES_NO_KERNELS
#include "b747_lanes.h"
#include "b747_policy.h"

namespace {

using namespace b747;

constexpr int kLanesBlock = 64;   // one wave per workgroup: the wave has the SIMD's whole register file

// *step_base += T in a launch of its own, ordered after the rollout kernel: inside that kernel a workgroup that
// starts late would read the advanced base.  (one lane's vector atomic, as k_policy_value's)
template <bool FAST>
__global__ __launch_bounds__(64) void k_step_base_advance(uint64_t *step_base, uint32_t advance)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_fetch_add(step_base, (uint64_t)advance, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_policy_act's sample and its log-probability (b747_policy.h), rounded as written there (that kernel is compiled
// without FMA contraction; so is this, also in the FAST unit: both paths then store the same action bits for the same
// mean and noise)
__device__ __forceinline__ void gaussian_sample(float mean, float log_std, float z, float &a, float &logp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    a = mean + expf(log_std) * z;
    // log N(a; mean, std) with a - mean = std * z
    logp = -0.5f * z * z - log_std - 0.918938533204672742f;
}

// OD: the policy's obs_dim (3 PID_LIKE, 5 SPEED_MODE).  Lanes past n step a copy of env n - 1 (the matrix cores need
// all 64 lanes) and store nothing: no rollout row, no env buffer, no episode book, no state0 slot.
// The body (b747_rollout_lanes_body.h) is shared with the population form (k_rollout_population,
// b747_rollout_population.h); without POP and REW `pa` is never read.
template <bool FAST, int OD>
__global__ __launch_bounds__(kLanesBlock) B747_NO_FMAC void k_rollout_lanes(b747_env_batch b, b747_env_config cfgc,
                                                                            Consts Cin, RolloutLanesArgs ra)
{
    constexpr bool POP = false, REW = false;
    constexpr RolloutPopArgs pa{0, 1, nullptr, nullptr};   // (named by the discarded branches of the body only)
#include "b747_rollout_lanes_body.h"
}

template <bool FAST>
void launch_rollout_lanes(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                          const RolloutLanesArgs &ra, int od, uint64_t *advance, hipStream_t s)
{
    const dim3 g((unsigned)((b.n + kLanesBlock - 1) / kLanesBlock)), blk(kLanesBlock);
    if (od == 3) hipLaunchKernelGGL((k_rollout_lanes<FAST, 3>), g, blk, 0, s, b, cfg, C, ra);
    else hipLaunchKernelGGL((k_rollout_lanes<FAST, 5>), g, blk, 0, s, b, cfg, C, ra);
    if (advance) hipLaunchKernelGGL((k_step_base_advance<FAST>), dim3(1), dim3(64), 0, s, advance, (uint32_t)ra.T);
}

}  // namespace
#endif  // B747_ROLLOUT_LANES_NO_KERNELS
