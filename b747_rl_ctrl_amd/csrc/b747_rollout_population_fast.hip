// b747_rollout_population_fast.hip -- the FAST instantiations of the population PPO rollout kernel
// (b747_rollout_population.h), under the same FMA contraction as b747_fast.hip.  MIXED batches run these too (as every
// one-wave kernel).
#pragma clang fp contract(fast)

#define B747_POLICY_NO_KERNELS   // the policy kernels live in b747_kernels.hip; this unit reuses actor_critic
#include "b747_rollout_population.h"

namespace b747 {

void launch_rollout_population_fast(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                                    const RolloutLanesArgs &ra, const RolloutPopArgs &pa, int od, uint64_t *advance,
                                    hipStream_t s)
{
    launch_rollout_population<true>(b, cfg, C, ra, pa, od, advance, s);
}

}  // namespace b747
