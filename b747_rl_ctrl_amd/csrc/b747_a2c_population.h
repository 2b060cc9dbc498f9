// b747_a2c_population.h -- one A2C step of every member of a population on the device.
//
// b747_a2c_update.h's step for n_policies members at once, member p = blockIdx.y of every kernel, as b747_ppo_update.h's
// member-batched kernels are to b747_ppo_epoch.  The launches of one chunk of members (kernels in
// b747_a2c_population.hip):
//   k_apop_adv_stats  b747_ppo_adv_stats_body.h with POP, LOSS = kUpdLossA2c; grid (kUpdAdvBlocks, members); launched
//                     with normalize_advantage only;
//   k_apop_grad<OD>   b747_ppo_grad_body.h with POP, LOSS = kUpdLossA2c: k_a2c_grad<OD>'s row, the member's vf_coef from
//                     its row of the device hyper-parameter table; grid (upd_n_wg(batch), members);
//   k_apop_reduce     b747_ppo_reduce_body.h with POP, the member's ent_coef and vf_coef from the table;
//   k_apop_opt        clip_grad_norm_ and the member's optimiser -- the table's B747_PPO_HYPER_OPTIMIZER column picks
//                     k_ppo_rmsprop's arithmetic (either flavour) or k_ppo_adam's -- with its max_grad_norm and lr;
//                     grid (1, members).
// A member's rows of the time-major buffers are not a range: row p of the index table `rows` [n_policies][rows_stride]
// names them, read as the PPO kernels read perm (UpdPopArgs::n_rows is the table's row stride here); the first `batch`
// entries of a row are the minibatch.  The workspace is b747_ppo_epoch_batched's: one slice of
// upd_pop_ws_bytes(od, batch) per member of a chunk.  The statistics row is k_a2c_reduce's, 8 floats per member.
// No floating-point atomics; nothing allocates, synchronises or reads a per-member value on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b747_a2c_update.h"

namespace b747 {

// The optimisers' shared scalars (a member's own -- max_grad_norm, lr, the kind -- are in the table)
struct UpdPopOpt {
    double rms_alpha, rms_eps, adam_beta1, adam_beta2, adam_eps;
};

// One member's optimiser state rows and step count, member 0's: state0 is RMSprop's sq or Adam's m, state1 Adam's v
struct UpdPopState {
    float *theta, *state0, *state1;
    int64_t *t;
};

// Launcher, defined in b747_a2c_population.hip (hidden: not part of the C ABI).  Arguments are validated by the caller;
// an obs_dim without kernels (with_obs_dim) gives hipErrorInvalidValue.  d.old_logp is not read.  Members in chunks of
// min(n_policies, workspace_bytes / upd_pop_ws_bytes(od, batch), kUpdPopMaxMembers); the first launch error ends the
// loop and is returned.
#define B747_HIDDEN __attribute__((visibility("hidden")))
B747_HIDDEN hipError_t launch_a2c_update_population(const UpdPopState &st, int n_policies, int64_t policy_stride, int od,
                                                    const UpdData &d, const int64_t *rows, int64_t rows_stride,
                                                    int64_t batch, bool normalize_advantage, const double *hyper_dev,
                                                    void *workspace, int64_t workspace_bytes, const UpdPopOpt &opt,
                                                    float *stats, hipStream_t s);
#undef B747_HIDDEN

}  // namespace b747
