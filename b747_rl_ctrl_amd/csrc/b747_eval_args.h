// b747_eval_args.h -- the argument block and the launchers of the evaluation-episode kernel (b747_eval.h): what
// b747_kernels.hip (the C ABI, b747_eval_episodes) shares with the two translation units that instantiate it.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/b747.h"
#include "b747_dynamics.h"

namespace b747 {

struct EvalArgs {
    const float *params;      // packed policy (b747_policy_pack), NULL = no policy: b.action held for the episode
    int32_t n_env_steps;
    int32_t sig_row;          // B747_SIG_* row of the scored signal
    double scale;             // series = scale * nan_to_num(signal)
    const double *y_base;     // [N] the command the series is scored against
    double error_band;
    float act_lo, act_hi;
    double *out;              // [B747_NEVAL][N]
};

// What the population form adds (b747_eval_population; k_eval_population, b747_eval.h)
struct PopArgs {
    int64_t policy_stride;    // floats from one packed policy to the next
    int32_t waves_per_policy; // envs_per_policy / 64: workgroup w flies policy w / waves_per_policy
    const double *pid_ss;     // [4][N] the env's own SS PID gains, NULL = Consts::PID_SS for every env
    const double *pid_cs;     // [4][N] likewise for the CS PID
};

// Defined in b747_eval_fast.hip / b747_eval_faithful.hip (hidden: not part of the C ABI); od = the policy's obs_dim
// (3 or 5), 0 = no policy
__attribute__((visibility("hidden"))) void launch_eval_episodes_fast(const b747_env_batch &b, const b747_env_config &cfg,
                                                                     const Consts &C, const EvalArgs &ea, int od,
                                                                     hipStream_t s);
__attribute__((visibility("hidden"))) void launch_eval_episodes_faithful(const b747_env_batch &b, const b747_env_config &cfg,
                                                                         const Consts &C, const EvalArgs &ea, int od,
                                                                         hipStream_t s);
__attribute__((visibility("hidden"))) void launch_eval_population_fast(const b747_env_batch &b, const b747_env_config &cfg,
                                                                       const Consts &C, const EvalArgs &ea,
                                                                       const PopArgs &pa, int od, hipStream_t s);
__attribute__((visibility("hidden"))) void launch_eval_population_faithful(const b747_env_batch &b,
                                                                           const b747_env_config &cfg, const Consts &C,
                                                                           const EvalArgs &ea, const PopArgs &pa, int od,
                                                                           hipStream_t s);
}  // namespace b747
