// b747_rollout_population.h -- P learners' stochastic PPO rollouts side by side in one launch
// (b747_ppo_rollout_population, include/b747.h).
//
// k_rollout_population is k_rollout_lanes (b747_rollout_lanes.h; the body is shared, b747_rollout_lanes_body.h) with
// four differences.  A policy per group of waves: workgroup (= wave) w reads ITS packed policy, at params +
// (w / waves_per_policy) * policy_stride -- a wave-uniform address, in the prologue's PolicyStage load and in the
// per-step fragment pointer alike; lanes past n copy env n - 1, which flies in the same wave and so under the same
// policy.  Reward constants per group (REW): the wave steps with a private configuration whose rew[0..7] are its
// group's row of rew_pop.  The value head always runs in the step loop (k_policy_value<3>'s deferred pass takes one
// policy for all rows), and once more after the last step, on the observation the kernel leaves in b.obs: last_val,
// the bootstrap value of GAE.  Instantiated by two translation units of its own,
// b747_rollout_population_faithful.hip and b747_rollout_population_fast.hip (as every one-wave kernel: new kernels
// inside an existing unit changed the code generated for the kernels already there).
#pragma once

#include "b747_rollout_lanes.h"

namespace {

using namespace b747;

template <bool FAST, int OD, bool REW>
__global__ __launch_bounds__(kLanesBlock) B747_NO_FMAC void k_rollout_population(b747_env_batch b, b747_env_config cfgc,
                                                                                 Consts Cin, RolloutLanesArgs ra,
                                                                                 RolloutPopArgs pa)
{
    constexpr bool POP = true;
#include "b747_rollout_lanes_body.h"
}

template <bool FAST>
void launch_rollout_population(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                               const RolloutLanesArgs &ra, const RolloutPopArgs &pa, int od, uint64_t *advance,
                               hipStream_t s)
{
    const dim3 g((unsigned)((b.n + kLanesBlock - 1) / kLanesBlock)), blk(kLanesBlock);
    const bool rew = pa.rew_pop != nullptr;
#define B747_LAUNCH_POP(OD, R) hipLaunchKernelGGL((k_rollout_population<FAST, OD, R>), g, blk, 0, s, b, cfg, C, ra, pa)
    if (od == 3) { if (rew) B747_LAUNCH_POP(3, true); else B747_LAUNCH_POP(3, false); }
    else { if (rew) B747_LAUNCH_POP(5, true); else B747_LAUNCH_POP(5, false); }
#undef B747_LAUNCH_POP
    if (advance) hipLaunchKernelGGL((k_step_base_advance<FAST>), dim3(1), dim3(64), 0, s, advance, (uint32_t)ra.T);
}

}  // namespace
