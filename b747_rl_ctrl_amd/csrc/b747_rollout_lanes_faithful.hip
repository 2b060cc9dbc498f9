// b747_rollout_lanes_faithful.hip -- the FAITHFUL instantiations of the one-wave PPO rollout kernel
// (b747_rollout_lanes.h): no FMA contraction (-ffp-contract=off, build.py), the DLL's roundings, as b747_kernels.hip.
#define B747_POLICY_NO_KERNELS   // the policy kernels live in b747_kernels.hip; this unit reuses actor_critic
#include "b747_rollout_lanes.h"

namespace b747 {

void launch_rollout_lanes_faithful(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                                   const RolloutLanesArgs &ra, int od, uint64_t *advance, hipStream_t s)
{
    launch_rollout_lanes<false>(b, cfg, C, ra, od, advance, s);
}

}  // namespace b747
