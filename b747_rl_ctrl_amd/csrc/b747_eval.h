// b747_eval.h -- whole evaluation episodes in one launch (b747_eval_episodes, include/b747.h).
//
// ControlTestCallback.calc_stepinfo (neural/callbacks.py:60-100) flies one episode per pitch reference with the
// deterministic policy and scores the recorded pitch with calc_stepinfo.  k_eval_episodes does that for 64 envs per
// wave without a history: the policy head (actor_critic<OD, 1>, b747_policy.h) runs in the step loop on the
// observations the last read-out left behind, the generic lane code of b747_lanes.h steps the env (every control
// type / mode, reward, limiter setting and n_sub that k_env_steps covers; run-time constants), and after every DLL
// step the chosen signal goes into the lane's StepInfoAcc (b747_stepinfo.h).  Only B747_NEVAL values per env leave
// the kernel.  Instantiated by two translation units of its own, b747_eval_faithful.hip and b747_eval_fast.hip (the
// FAITHFUL / FAST split of b747_kernels.hip / b747_fast.hip): compiled inside those two, the new kernels changed the
// register allocation and LDS-read scheduling of kernels already there (k_rollout_split<true, ...>).
#pragma once

#include "b747_lanes.h"
#include "b747_policy.h"
#include "b747_stepinfo.h"

#include "b747_eval_args.h"

namespace {

using namespace b747;

// The per-DLL-step hook of env_step_lane: one sample of the scored series per DLL step
struct EvalPush {
    static constexpr bool kEveryStep = true;
    StepInfoAcc &acc;
    int32_t &len;
    int row;
    double scale;
    __device__ __forceinline__ void operator()(const double *sg, int sst) const
    {
        acc.push(scale * nan_to_num(sg[row * sst]), sg[S_SIM_TIME * sst]);
        len += 1;
    }
};

constexpr int kEvalBlock = 64;   // one wave per workgroup: the wave has the SIMD's whole register file
// OD: the policy's obs_dim (3 PID_LIKE, 5 SPEED_MODE), 0 = no policy.  An env's episode ends at its first done or
// after n_env_steps; from then on the lane is frozen (no samples, no return, its state as at the done) while the
// wave's loop runs on for the lanes still live.  Lanes past n step a copy of env n - 1 (the matrix cores need all 64
// lanes) and store nothing.
//
// The body (b747_eval_body.h) is shared with the population form (k_eval_population, below).  POP: workgroup
// (= wave) w reads ITS policy, at params + (w / waves_per_policy) * policy_stride -- a wave-uniform address, in the
// prologue's PolicyStage load and in the per-step fragment pointer alike; lanes past n copy env n - 1, which flies in
// the same wave and so under the same policy.  GAINS: the lane steps with a private Consts whose PID_SS / PID_CS are
// its own row of pa.pid_ss / pa.pid_cs ([4][N], each nullable: a NULL pointer keeps the batch constant); the gains
// enter the dynamics in pass() only (b747_dynamics.h), resets do not read them.  Without POP and GAINS `pa` is never
// read.
template <bool FAST, int OD>
__global__ __launch_bounds__(kEvalBlock) B747_NO_FMAC void k_eval_episodes(b747_env_batch b, b747_env_config cfgc,
                                                                           Consts Cin, EvalArgs ea)
{
    constexpr bool POP = false, GAINS = false;
    constexpr PopArgs pa{0, 1, nullptr, nullptr};   // (named by the discarded branches of the body only)
#include "b747_eval_body.h"
}

// The population form (b747_eval_population): a policy per group of waves, PID gains per env
template <bool FAST, int OD, bool GAINS>
__global__ __launch_bounds__(kEvalBlock) B747_NO_FMAC void k_eval_population(b747_env_batch b, b747_env_config cfgc,
                                                                             Consts Cin, EvalArgs ea, PopArgs pa)
{
    constexpr bool POP = OD != 0;
#include "b747_eval_body.h"
}

template <bool FAST>
void launch_eval_population(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C, const EvalArgs &ea,
                            const PopArgs &pa, int od, hipStream_t s)
{
    const dim3 g((unsigned)((b.n + kEvalBlock - 1) / kEvalBlock)), blk(kEvalBlock);
    const bool gains = pa.pid_ss || pa.pid_cs;
#define B747_LAUNCH_POP(OD, G) hipLaunchKernelGGL((k_eval_population<FAST, OD, G>), g, blk, 0, s, b, cfg, C, ea, pa)
    if (od == 3) { if (gains) B747_LAUNCH_POP(3, true); else B747_LAUNCH_POP(3, false); }
    else if (od == 5) { if (gains) B747_LAUNCH_POP(5, true); else B747_LAUNCH_POP(5, false); }
    else if (gains) B747_LAUNCH_POP(0, true);
    else hipLaunchKernelGGL((k_eval_episodes<FAST, 0>), g, blk, 0, s, b, cfg, C, ea);   // no policy, no gains: §10's kernel
#undef B747_LAUNCH_POP
}

template <bool FAST>
void launch_eval_episodes(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C, const EvalArgs &ea,
                          int od, hipStream_t s)
{
    const dim3 g((unsigned)((b.n + kEvalBlock - 1) / kEvalBlock)), blk(kEvalBlock);
    if (od == 3) hipLaunchKernelGGL((k_eval_episodes<FAST, 3>), g, blk, 0, s, b, cfg, C, ea);
    else if (od == 5) hipLaunchKernelGGL((k_eval_episodes<FAST, 5>), g, blk, 0, s, b, cfg, C, ea);
    else hipLaunchKernelGGL((k_eval_episodes<FAST, 0>), g, blk, 0, s, b, cfg, C, ea);
}

}  // namespace
