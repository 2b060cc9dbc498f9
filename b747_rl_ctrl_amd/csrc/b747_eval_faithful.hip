// b747_eval_faithful.hip -- the FAITHFUL instantiations of the evaluation-episode kernel (b747_eval.h): no FMA
// contraction (-ffp-contract=off, build.py), the DLL's roundings, as b747_kernels.hip.
#define B747_POLICY_NO_KERNELS   // the policy kernels live in b747_kernels.hip; this unit reuses actor_critic
#include "b747_eval.h"

namespace b747 {

void launch_eval_episodes_faithful(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                                   const EvalArgs &ea, int od, hipStream_t s)
{
    launch_eval_episodes<false>(b, cfg, C, ea, od, s);
}

void launch_eval_population_faithful(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                                     const EvalArgs &ea, const PopArgs &pa, int od, hipStream_t s)
{
    launch_eval_population<false>(b, cfg, C, ea, pa, od, s);
}

}  // namespace b747
