// b747_rollout_population_faithful.hip -- the FAITHFUL instantiations of the population PPO rollout kernel
// (b747_rollout_population.h): no FMA contraction (-ffp-contract=off, build.py), the DLL's roundings, as
// b747_kernels.hip.
#define B747_POLICY_NO_KERNELS   // the policy kernels live in b747_kernels.hip; this unit reuses actor_critic
#include "b747_rollout_population.h"

namespace b747 {

void launch_rollout_population_faithful(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                                        const RolloutLanesArgs &ra, const RolloutPopArgs &pa, int od,
                                        uint64_t *advance, hipStream_t s)
{
    launch_rollout_population<false>(b, cfg, C, ra, pa, od, advance, s);
}

}  // namespace b747
