// b747_eval_fast.hip -- the FAST instantiations of the evaluation-episode kernel (b747_eval.h), under the same FMA
// contraction as b747_fast.hip.  MIXED batches run these too (as every one-wave kernel).
#pragma clang fp contract(fast)

#define B747_POLICY_NO_KERNELS   // the policy kernels live in b747_kernels.hip; this unit reuses actor_critic
#include "b747_eval.h"

namespace b747 {

void launch_eval_episodes_fast(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C, const EvalArgs &ea,
                               int od, hipStream_t s)
{
    launch_eval_episodes<true>(b, cfg, C, ea, od, s);
}

void launch_eval_population_fast(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C, const EvalArgs &ea,
                                 const PopArgs &pa, int od, hipStream_t s)
{
    launch_eval_population<true>(b, cfg, C, ea, pa, od, s);
}

}  // namespace b747
