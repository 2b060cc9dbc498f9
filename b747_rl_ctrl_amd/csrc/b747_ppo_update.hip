// b747_ppo_update.hip -- the fused PPO minibatch update (b747_ppo_update.h): its kernels and their launchers, a
// translation unit of their own so that the kernels of the other units keep their generated code.
#define B747_POLICY_NO_KERNELS   // PolicyLayout only
#include "b747_ppo_update.h"

namespace b747 {

namespace {

// (the attribute belongs to the current device's copy of the kernel; a host-side setting, no stream work)
template <int OD>
hipError_t grad_lds_limit()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ppo_grad<OD>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, UpdLds<OD>::bytes);
}

// The three gradient launches of one minibatch (grad_lds_limit<OD>() has been called on this device)
template <int OD>
hipError_t grad_launch(const float *theta, const float *obs, const float *act, const float *old_logp, const float *adv,
                       const float *ret, const int64_t *idx, int64_t batch, double clip_range, double ent_coef,
                       double vf_coef, void *workspace, float *grad, float *stats, hipStream_t s)
{
    constexpr int P = PolicyLayout::of(OD).total;
    char *ws = static_cast<char *>(workspace);
    double *adv_part = reinterpret_cast<double *>(ws + upd_ws_adv());
    double *spart = reinterpret_cast<double *>(ws + upd_ws_sums());
    float *gpart = reinterpret_cast<float *>(ws + upd_ws_grad());
    const int64_t tiles = (batch + kUpdTile - 1) / kUpdTile, want = (tiles + 1) / 2;   // (two tiles in flight per workgroup and net)
    const int n_wg = (int)(want < kUpdMaxWG ? want : kUpdMaxWG);
    hipLaunchKernelGGL(k_ppo_adv_stats, dim3(kUpdAdvBlocks), dim3(256), 0, s, adv, idx, batch, adv_part);
    hipLaunchKernelGGL(k_ppo_grad<OD>, dim3(n_wg), dim3(256), UpdLds<OD>::bytes, s, theta, obs, act, old_logp, adv, ret,
                       idx, batch, clip_range, vf_coef, adv_part, gpart, spart);
    hipLaunchKernelGGL(k_ppo_reduce, dim3((P + 1 + 255) / 256), dim3(256), 0, s, gpart, spart, n_wg, P,
                       PolicyLayout::of(OD).ba, PolicyLayout::of(OD).bv, PolicyLayout::of(OD).log_std, theta, batch, (float)ent_coef, (float)vf_coef, grad, stats);
    return hipGetLastError();
}

template <int OD>
hipError_t grad_od(const float *theta, const float *obs, const float *act, const float *old_logp, const float *adv,
                   const float *ret, const int64_t *idx, int64_t batch, double clip_range, double ent_coef,
                   double vf_coef, void *workspace, float *grad, float *stats, hipStream_t s)
{
    const hipError_t attr = grad_lds_limit<OD>();   // (per call)
    if (attr != hipSuccess) return attr;
    return grad_launch<OD>(theta, obs, act, old_logp, adv, ret, idx, batch, clip_range, ent_coef, vf_coef, workspace, grad,
                           stats, s);
}

// b747_ppo_epoch's loop: minibatch j is grad_od's launches on perm + j batch_size and stats + 8 j, then
// launch_ppo_adam with grad_scale 1 -- the launches of the two-call path in its order, the LDS limit raised once
template <int OD>
hipError_t epoch_od(float *theta, const float *obs, const float *act, const float *old_logp, const float *adv,
                    const float *ret, const int64_t *perm, int64_t n_rows, int64_t batch_size, double clip_range,
                    double ent_coef, double vf_coef, void *workspace, float *grad, float *m, float *v, int64_t *t,
                    double max_grad_norm, double lr, double beta1, double beta2, double eps, float *stats, hipStream_t s)
{
    hipError_t e = grad_lds_limit<OD>();
    if (e != hipSuccess) return e;
    for (int64_t at = 0; at < n_rows; at += batch_size, stats += kUpdStats) {
        const int64_t batch = n_rows - at < batch_size ? n_rows - at : batch_size;
        e = grad_launch<OD>(theta, obs, act, old_logp, adv, ret, perm + at, batch, clip_range, ent_coef, vf_coef, workspace,
                            grad, stats, s);
        if (e != hipSuccess) return e;
        e = launch_ppo_adam(theta, m, v, t, grad, PolicyLayout::of(OD).total, 1.0, max_grad_norm, lr, beta1, beta2, eps, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// b747_ppo_epoch_batched's loops: members in chunks of as many slices as the workspace holds; a chunk's minibatch j is
// the four launches of epoch_od's minibatch j with the members on blockIdx.y.  The pointers passed are those of the
// chunk's first member; the kernels add the member's distance (UpdPopArgs).
template <int OD>
hipError_t epoch_batched_od(float *theta, int n_policies, int64_t policy_stride, const float *obs, const float *act,
                            const float *old_logp, const float *adv, const float *ret, const int64_t *perm,
                            int64_t n_rows, int64_t batch_size, double clip_range, double ent_coef, double vf_coef,
                            void *workspace, int64_t workspace_bytes, float *m, float *v, int64_t *t,
                            double max_grad_norm, const double *lr, double beta1, double beta2, double eps, float *stats,
                            hipStream_t s)
{
    constexpr PolicyLayout L = PolicyLayout::of(OD);
    constexpr int P = L.total;
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pop_grad<OD>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, UpdLds<OD>::bytes);
    if (attr != hipSuccess) return attr;
    const int64_t per = upd_pop_ws_bytes(OD, batch_size), n_mb = (n_rows + batch_size - 1) / batch_size;
    int64_t chunk = workspace_bytes / per;
    if (chunk > n_policies) chunk = n_policies;
    if (chunk > kUpdPopMaxMembers) chunk = kUpdPopMaxMembers;
    const UpdPopArgs pa{policy_stride, P, n_rows, per, n_mb * kUpdStats};
    char *ws = static_cast<char *>(workspace);
    double *adv_part = reinterpret_cast<double *>(ws + upd_ws_adv());
    double *spart = reinterpret_cast<double *>(ws + upd_ws_sums());
    float *gpart = reinterpret_cast<float *>(ws + upd_pop_ws_grad(batch_size));
    float *grad = reinterpret_cast<float *>(ws + upd_pop_ws_out(OD, batch_size));
    for (int64_t c0 = 0; c0 < n_policies; c0 += chunk) {
        const unsigned members = (unsigned)(n_policies - c0 < chunk ? n_policies - c0 : chunk);
        float *th = theta + c0 * policy_stride, *st = stats + c0 * n_mb * kUpdStats;
        const int64_t *pm = perm + c0 * n_rows;
        for (int64_t at = 0; at < n_rows; at += batch_size, st += kUpdStats) {
            const int64_t batch = n_rows - at < batch_size ? n_rows - at : batch_size;
            const int n_wg = upd_n_wg(batch);
            hipLaunchKernelGGL(k_pop_adv_stats, dim3(kUpdAdvBlocks, members), dim3(256), 0, s, adv, pm + at, batch,
                               adv_part, pa);
            hipLaunchKernelGGL(k_pop_grad<OD>, dim3(n_wg, members), dim3(256), UpdLds<OD>::bytes, s, th, obs, act, old_logp,
                               adv, ret, pm + at, batch, clip_range, vf_coef, adv_part, gpart, spart, pa);
            hipLaunchKernelGGL(k_pop_reduce, dim3((P + 1 + 255) / 256, members), dim3(256), 0, s, gpart, spart, n_wg, P,
                               L.ba, L.bv, L.log_std, th, batch, (float)ent_coef, (float)vf_coef, grad, st, pa);
            hipLaunchKernelGGL(k_pop_adam, dim3(1, members), dim3(kUpdAdamBlock), 0, s, th, m + c0 * P, v + c0 * P, t + c0,
                               grad, (int64_t)P, 1.0, max_grad_norm, lr + c0, beta1, beta2, eps, pa);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_ppo_grad(const float *theta, int od, const float *obs, const float *act, const float *old_logp,
                           const float *adv, const float *ret, const int64_t *idx, int64_t batch, double clip_range,
                           double ent_coef, double vf_coef, void *workspace, float *grad, float *stats, hipStream_t s)
{
#define B747_GRAD(OD)                                                                                              \
    case OD:                                                                                                       \
        return grad_od<OD>(theta, obs, act, old_logp, adv, ret, idx, batch, clip_range, ent_coef, vf_coef, workspace, \
                           grad, stats, s)
    switch (od) {
        B747_GRAD(3);
        B747_GRAD(5);
        B747_GRAD(7);
        B747_GRAD(8);
        B747_GRAD(10);
    default: return hipErrorInvalidValue;
    }
#undef B747_GRAD
}

hipError_t launch_ppo_adam(float *theta, float *m, float *v, int64_t *t, const float *grad, int64_t n_params,
                           double grad_scale, double max_grad_norm, double lr, double beta1, double beta2, double eps,
                           hipStream_t s)
{
    hipLaunchKernelGGL(k_ppo_adam, dim3(1), dim3(kUpdAdamBlock), 0, s, theta, m, v, t, grad, n_params, grad_scale,
                       max_grad_norm, lr, beta1, beta2, eps);
    return hipGetLastError();
}

hipError_t launch_ppo_epoch(float *theta, int od, const float *obs, const float *act, const float *old_logp,
                            const float *adv, const float *ret, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                            double clip_range, double ent_coef, double vf_coef, void *workspace, float *grad, float *m,
                            float *v, int64_t *t, double max_grad_norm, double lr, double beta1, double beta2,
                            double eps, float *stats, hipStream_t s)
{
#define B747_EPOCH(OD)                                                                                               \
    case OD:                                                                                                         \
        return epoch_od<OD>(theta, obs, act, old_logp, adv, ret, perm, n_rows, batch_size, clip_range, ent_coef, vf_coef, \
                            workspace, grad, m, v, t, max_grad_norm, lr, beta1, beta2, eps, stats, s)
    switch (od) {
        B747_EPOCH(3);
        B747_EPOCH(5);
        B747_EPOCH(7);
        B747_EPOCH(8);
        B747_EPOCH(10);
    default: return hipErrorInvalidValue;
    }
#undef B747_EPOCH
}

hipError_t launch_ppo_epoch_batched(float *theta, int n_policies, int64_t policy_stride, int od, const float *obs,
                                    const float *act, const float *old_logp, const float *adv, const float *ret,
                                    const int64_t *perm, int64_t n_rows, int64_t batch_size, double clip_range,
                                    double ent_coef, double vf_coef, void *workspace, int64_t workspace_bytes, float *m,
                                    float *v, int64_t *t, double max_grad_norm, const double *lr, double beta1,
                                    double beta2, double eps, float *stats, hipStream_t s)
{
#define B747_EPOCH_BATCHED(OD)                                                                                        \
    case OD:                                                                                                          \
        return epoch_batched_od<OD>(theta, n_policies, policy_stride, obs, act, old_logp, adv, ret, perm, n_rows,     \
                                    batch_size, clip_range, ent_coef, vf_coef, workspace, workspace_bytes, m, v, t,   \
                                    max_grad_norm, lr, beta1, beta2, eps, stats, s)
    switch (od) {
        B747_EPOCH_BATCHED(3);
        B747_EPOCH_BATCHED(5);
        B747_EPOCH_BATCHED(7);
        B747_EPOCH_BATCHED(8);
        B747_EPOCH_BATCHED(10);
    default: return hipErrorInvalidValue;
    }
#undef B747_EPOCH_BATCHED
}

}  // namespace b747
