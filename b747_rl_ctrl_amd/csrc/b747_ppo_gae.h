// b747_ppo_gae.h -- generalized advantage estimation over a time-major rollout in one launch (b747_ppo_gae,
// include/b747.h).  The kernel lives in b747_ppo_gae.hip; this is its launcher's declaration.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace b747 {

#ifndef B747_GAE_BLOCK
#define B747_GAE_BLOCK 64    // lanes (envs) per workgroup; measured against 256 (profiles/ppo_epoch.json)
#endif
#ifndef B747_GAE_UNROLL
#define B747_GAE_UNROLL 16   // time steps per chunk, two chunks' loads in flight; measured against 1, 4, 8 and 32 (ibid.)
#endif
constexpr int kGaeBlock = B747_GAE_BLOCK;
constexpr int kGaeUnroll = B747_GAE_UNROLL;

// Hidden: not part of the C ABI.  Arguments are validated by the caller (T >= 1, 1 <= N <= kGaeBlock * INT32_MAX).
__attribute__((visibility("hidden"))) hipError_t launch_ppo_gae(const float *rew, const float *val, const uint8_t *done,
                                                                const float *last_value, int32_t T, int64_t N,
                                                                double gamma, double gae_lambda, float *adv, float *ret,
                                                                hipStream_t s);
// b747_ppo_gae_population's launch: env i takes gamma and gae_lambda from row i / envs_per_policy of the device table
// hyper_dev (include/b747.h B747_PPO_HYPER_*).  Validated by the caller as above, and envs_per_policy a positive
// multiple of 64 with N at most n_policies envs_per_policy (no row past the table is read).
__attribute__((visibility("hidden"))) hipError_t launch_ppo_gae_population(const float *rew, const float *val,
                                                                           const uint8_t *done, const float *last_value,
                                                                           int32_t T, int64_t N, int32_t envs_per_policy,
                                                                           const double *hyper_dev, float *adv,
                                                                           float *ret, hipStream_t s);

}  // namespace b747
