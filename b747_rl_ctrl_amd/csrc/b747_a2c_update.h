// b747_a2c_update.h -- one A2C step on the device: loss, gradient, clip and RMSprop / Adam.
//
// SB3 1.4 A2C.train for the policy every kernel here is written for (b747_ppo_update.h): ONE gradient step over the
// whole rollout, loss = mean(-A logp) + ent_coef (-entropy) + vf_coef mean((ret - value)^2), A the advantage or, with
// normalize_advantage, (adv - mean) / (std + 1e-8) over the batch.  The launches (kernels in b747_a2c_update.hip):
//   k_a2c_adv_stats   b747_ppo_adv_stats_body.h -- k_ppo_adv_stats' text with idx allowed to be NULL; launched with
//                     normalize_advantage only;
//   k_a2c_grad<OD>    b747_ppo_grad_body.h with LOSS = kUpdLossA2c: k_ppo_grad's staging, forward (fp64), matrix-core
//                     backward, transpositions and flush; upd_tiles' A2C row -- no ratio, no clip, g_logp = -A / B on
//                     every row; the same grid (upd_n_wg) and workspace (b747_ppo_update_workspace);
//   k_a2c_reduce      b747_ppo_reduce_body.h, unchanged text;
//   k_ppo_rmsprop     clip_grad_norm_ + RMSprop on the flat vector (torch.optim.RMSprop or SB3's RMSpropTFLike), or
//                     k_ppo_adam through launch_ppo_adam as it stands.
// The statistics row is k_ppo_reduce's, 8 floats: [0] policy loss mean(-A logp), [1] value loss, [2] entropy loss,
// [3] 0, [4] 0, [5] mean |A logp| (the magnitude of the terms the policy loss sums: abs_a_ratio's role), [6] 0,
// [7] the loss.  No floating-point atomics: the same inputs give the same bits.  Nothing allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b747_ppo_update.h"

namespace b747 {

// RMSprop's scalars (no momentum, not centred, no weight decay).  tf_like: the step divides by sqrt(sq + eps) (SB3's
// RMSpropTFLike; its state starts at ones, the caller's fill) instead of sqrt(sq) + eps (torch.optim.RMSprop)
struct UpdRms {
    double max_grad_norm, alpha, eps;
    bool tf_like;
};

// Launchers, defined in b747_a2c_update.hip (hidden: not part of the C ABI).  Arguments are validated by the caller;
// an obs_dim without kernels (with_obs_dim) gives hipErrorInvalidValue.  d.old_logp is not read.  idx may be NULL:
// the rows 0 .. batch - 1.
#define B747_HIDDEN __attribute__((visibility("hidden")))
B747_HIDDEN hipError_t launch_a2c_grad(const float *theta, int od, const UpdData &d, const int64_t *idx, int64_t batch,
                                       bool normalize_advantage, double ent_coef, double vf_coef, void *workspace,
                                       float *grad, float *stats, hipStream_t s);
B747_HIDDEN hipError_t launch_ppo_rmsprop(float *theta, float *sq, int64_t *t, const float *grad, int64_t n_params,
                                          double grad_scale, const UpdRms &rms, double lr, hipStream_t s);
#undef B747_HIDDEN

}  // namespace b747
