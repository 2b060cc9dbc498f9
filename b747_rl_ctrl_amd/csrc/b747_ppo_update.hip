// b747_ppo_update.hip -- the fused PPO minibatch update (b747_ppo_update.h): its kernels and their launchers, a
// translation unit of their own so that the kernels of the other units keep their generated code.
#define B747_POLICY_NO_KERNELS   // PolicyLayout only
#include "b747_ppo_update.h"

namespace b747 {

namespace {

// The dynamic-LDS limit of k_ppo_grad<OD> or k_pop_grad<OD> (the attribute belongs to the current device's copy of the
// kernel; a host-side setting, no stream work)
template <int OD, class K>
hipError_t grad_lds_limit(K *kernel)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               UpdLds<OD>::bytes);
}

// The three gradient launches of one minibatch (grad_lds_limit<OD>(&k_ppo_grad<OD>) has been called on this device)
template <int OD>
hipError_t grad_launch(const float *theta, const UpdData &d, const int64_t *idx, int64_t batch, const UpdLoss &loss,
                       void *workspace, float *grad, float *stats, hipStream_t s)
{
    constexpr PolicyLayout L = PolicyLayout::of(OD);
    char *ws = static_cast<char *>(workspace);
    double *adv_part = reinterpret_cast<double *>(ws + upd_ws_adv());
    double *spart = reinterpret_cast<double *>(ws + upd_ws_sums());
    float *gpart = reinterpret_cast<float *>(ws + upd_ws_grad());
    // upd_n_wg(batch), spelled out: tests/test_gpu_ppo_update_grid.py reads the grid's formula from this file
    const int64_t tiles = (batch + kUpdTile - 1) / kUpdTile, want = (tiles + 1) / 2;   // (two tiles in flight per workgroup and net)
    const int n_wg = (int)(want < kUpdMaxWG ? want : kUpdMaxWG);
    hipLaunchKernelGGL(k_ppo_adv_stats, dim3(kUpdAdvBlocks), dim3(256), 0, s, d.adv, idx, batch, adv_part);
    hipLaunchKernelGGL(k_ppo_grad<OD>, dim3(n_wg), dim3(256), UpdLds<OD>::bytes, s, theta, d.obs, d.act, d.old_logp, d.adv,
                       d.ret, idx, batch, loss.clip_range, loss.vf_coef, adv_part, gpart, spart);
    hipLaunchKernelGGL(k_ppo_reduce, dim3((L.total + 1 + 255) / 256), dim3(256), 0, s, gpart, spart, n_wg, L.total, L.ba,
                       L.bv, L.log_std, theta, batch, (float)loss.ent_coef, (float)loss.vf_coef, grad, stats);
    return hipGetLastError();
}

// b747_ppo_epoch's loop: minibatch j is grad_launch's launches on perm + j batch_size and stats + 8 j, then
// launch_ppo_adam with grad_scale 1 -- the launches of the two-call path in its order, the LDS limit raised once
template <int OD>
hipError_t epoch_od(const UpdState &st, const UpdData &d, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                    const UpdLoss &loss, void *workspace, float *grad, const UpdAdam &adam, double lr, float *stats,
                    hipStream_t s)
{
    hipError_t e = grad_lds_limit<OD>(&k_ppo_grad<OD>);
    if (e != hipSuccess) return e;
    for (int64_t at = 0; at < n_rows; at += batch_size, stats += kUpdStats) {
        const int64_t batch = n_rows - at < batch_size ? n_rows - at : batch_size;
        e = grad_launch<OD>(st.theta, d, perm + at, batch, loss, workspace, grad, stats, s);
        if (e != hipSuccess) return e;
        e = launch_ppo_adam(st, grad, PolicyLayout::of(OD).total, 1.0, adam, lr, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// b747_ppo_epoch_batched's loops: members in chunks of as many slices as the workspace holds; a chunk's minibatch j is
// the four launches of epoch_od's minibatch j with the members on blockIdx.y.  The pointers passed are those of the
// chunk's first member; the kernels add the member's distance (UpdPopArgs).
template <int OD>
hipError_t epoch_batched_od(const UpdState &st, int n_policies, int64_t policy_stride, const UpdData &d,
                            const int64_t *perm, int64_t n_rows, int64_t batch_size, const UpdLoss &loss,
                            void *workspace, int64_t workspace_bytes, const UpdAdam &adam, const double *lr,
                            float *stats, hipStream_t s)
{
    constexpr PolicyLayout L = PolicyLayout::of(OD);
    constexpr int P = L.total;
    const hipError_t attr = grad_lds_limit<OD>(&k_pop_grad<OD>);
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
        float *th = st.theta + c0 * policy_stride, *row = stats + c0 * n_mb * kUpdStats;
        const int64_t *pm = perm + c0 * n_rows;
        for (int64_t at = 0; at < n_rows; at += batch_size, row += kUpdStats) {
            const int64_t batch = n_rows - at < batch_size ? n_rows - at : batch_size;
            const int n_wg = upd_n_wg(batch);
            hipLaunchKernelGGL(k_pop_adv_stats, dim3(kUpdAdvBlocks, members), dim3(256), 0, s, d.adv, pm + at, batch,
                               adv_part, pa);
            hipLaunchKernelGGL(k_pop_grad<OD>, dim3(n_wg, members), dim3(256), UpdLds<OD>::bytes, s, th, d.obs, d.act,
                               d.old_logp, d.adv, d.ret, pm + at, batch, loss.clip_range, loss.vf_coef, adv_part, gpart,
                               spart, pa);
            hipLaunchKernelGGL(k_pop_reduce, dim3((P + 1 + 255) / 256, members), dim3(256), 0, s, gpart, spart, n_wg, P,
                               L.ba, L.bv, L.log_std, th, batch, (float)loss.ent_coef, (float)loss.vf_coef, grad, row, pa);
            hipLaunchKernelGGL(k_pop_adam, dim3(1, members), dim3(kUpdAdamBlock), 0, s, th, st.m + c0 * P, st.v + c0 * P,
                               st.t + c0, grad, (int64_t)P, 1.0, adam.max_grad_norm, lr + c0, adam.beta1, adam.beta2,
                               adam.eps, pa);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// b747_ppo_epoch_batched_hyper's loops: epoch_batched_od's chunks, grids and launch order with the k_hyp_* kernels,
// which read their member's hyper-parameters from the device table.  The table pointer passed is the row of the
// chunk's first member (as lr + c0 above); the kernels add blockIdx.y rows.
template <int OD>
hipError_t epoch_batched_hyper_od(const UpdState &st, int n_policies, int64_t policy_stride, const UpdData &d,
                                  const int64_t *perm, int64_t n_rows, int64_t batch_size, const double *hyper_dev,
                                  void *workspace, int64_t workspace_bytes, const UpdAdam &adam, float *stats,
                                  hipStream_t s)
{
    constexpr PolicyLayout L = PolicyLayout::of(OD);
    constexpr int P = L.total;
    const hipError_t attr = grad_lds_limit<OD>(&k_hyp_grad<OD>);
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
        float *th = st.theta + c0 * policy_stride, *row = stats + c0 * n_mb * kUpdStats;
        const int64_t *pm = perm + c0 * n_rows;
        const double *hyp = hyper_dev + c0 * B747_PPO_HYPER_COLS;
        for (int64_t at = 0; at < n_rows; at += batch_size, row += kUpdStats) {
            const int64_t batch = n_rows - at < batch_size ? n_rows - at : batch_size;
            const int n_wg = upd_n_wg(batch);
            hipLaunchKernelGGL(k_pop_adv_stats, dim3(kUpdAdvBlocks, members), dim3(256), 0, s, d.adv, pm + at, batch,
                               adv_part, pa);
            hipLaunchKernelGGL(k_hyp_grad<OD>, dim3(n_wg, members), dim3(256), UpdLds<OD>::bytes, s, th, d.obs, d.act,
                               d.old_logp, d.adv, d.ret, pm + at, batch, hyp, adv_part, gpart, spart, pa);
            hipLaunchKernelGGL(k_hyp_reduce, dim3((P + 1 + 255) / 256, members), dim3(256), 0, s, gpart, spart, n_wg, P,
                               L.ba, L.bv, L.log_std, th, batch, hyp, grad, row, pa);
            hipLaunchKernelGGL(k_hyp_adam, dim3(1, members), dim3(kUpdAdamBlock), 0, s, th, st.m + c0 * P, st.v + c0 * P,
                               st.t + c0, grad, (int64_t)P, 1.0, hyp, adam.beta1, adam.beta2, adam.eps, pa);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_ppo_grad(const float *theta, int od, const UpdData &d, const int64_t *idx, int64_t batch,
                           const UpdLoss &loss, void *workspace, float *grad, float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto OD) {
        const hipError_t attr = grad_lds_limit<OD()>(&k_ppo_grad<OD()>);   // (per call)
        if (attr != hipSuccess) return attr;
        return grad_launch<OD()>(theta, d, idx, batch, loss, workspace, grad, stats, s);
    });
}

hipError_t launch_ppo_adam(const UpdState &st, const float *grad, int64_t n_params, double grad_scale,
                           const UpdAdam &adam, double lr, hipStream_t s)
{
    hipLaunchKernelGGL(k_ppo_adam, dim3(1), dim3(kUpdAdamBlock), 0, s, st.theta, st.m, st.v, st.t, grad, n_params,
                       grad_scale, adam.max_grad_norm, lr, adam.beta1, adam.beta2, adam.eps);
    return hipGetLastError();
}

hipError_t launch_ppo_epoch(const UpdState &st, int od, const UpdData &d, const int64_t *perm, int64_t n_rows,
                            int64_t batch_size, const UpdLoss &loss, void *workspace, float *grad, const UpdAdam &adam,
                            double lr, float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto OD) {
        return epoch_od<OD()>(st, d, perm, n_rows, batch_size, loss, workspace, grad, adam, lr, stats, s);
    });
}

hipError_t launch_ppo_epoch_population(const UpdState &st, int n_policies, int64_t policy_stride, int od,
                                       const UpdData &d, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                                       const UpdLoss &loss, void *workspace, float *grad, const UpdAdam &adam,
                                       const double *lr, float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto OD) {
        constexpr int64_t P = PolicyLayout::of(OD()).total;
        const int64_t n_mb = (n_rows + batch_size - 1) / batch_size;
        for (int64_t p = 0; p < n_policies; ++p) {
            const UpdState member{st.theta + p * policy_stride, st.m + p * P, st.v + p * P, st.t + p};
            const hipError_t e = epoch_od<OD()>(member, d, perm + p * n_rows, n_rows, batch_size, loss, workspace, grad,
                                                adam, lr[p], stats + p * n_mb * kUpdStats, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

hipError_t launch_ppo_epoch_batched(const UpdState &st, int n_policies, int64_t policy_stride, int od, const UpdData &d,
                                    const int64_t *perm, int64_t n_rows, int64_t batch_size, const UpdLoss &loss,
                                    void *workspace, int64_t workspace_bytes, const UpdAdam &adam, const double *lr,
                                    float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto OD) {
        return epoch_batched_od<OD()>(st, n_policies, policy_stride, d, perm, n_rows, batch_size, loss, workspace,
                                      workspace_bytes, adam, lr, stats, s);
    });
}

// (adam.max_grad_norm is not read by the two below: the table's column takes its place)
hipError_t launch_ppo_epoch_population_hyper(const UpdState &st, int n_policies, int64_t policy_stride, int od,
                                             const UpdData &d, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                                             const double *hyper, void *workspace, float *grad, const UpdAdam &adam,
                                             float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto OD) {
        constexpr int64_t P = PolicyLayout::of(OD()).total;
        const int64_t n_mb = (n_rows + batch_size - 1) / batch_size;
        for (int64_t p = 0; p < n_policies; ++p) {
            const double *h = hyper + p * B747_PPO_HYPER_COLS;
            const UpdState member{st.theta + p * policy_stride, st.m + p * P, st.v + p * P, st.t + p};
            const UpdLoss loss{h[B747_PPO_HYPER_CLIP_RANGE], h[B747_PPO_HYPER_ENT_COEF], h[B747_PPO_HYPER_VF_COEF]};
            const UpdAdam mine{h[B747_PPO_HYPER_MAX_GRAD_NORM], adam.beta1, adam.beta2, adam.eps};
            const hipError_t e = epoch_od<OD()>(member, d, perm + p * n_rows, n_rows, batch_size, loss, workspace, grad,
                                                mine, h[B747_PPO_HYPER_LR], stats + p * n_mb * kUpdStats, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

hipError_t launch_ppo_epoch_batched_hyper(const UpdState &st, int n_policies, int64_t policy_stride, int od,
                                          const UpdData &d, const int64_t *perm, int64_t n_rows, int64_t batch_size,
                                          const double *hyper_dev, void *workspace, int64_t workspace_bytes,
                                          const UpdAdam &adam, float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto OD) {
        return epoch_batched_hyper_od<OD()>(st, n_policies, policy_stride, d, perm, n_rows, batch_size, hyper_dev,
                                            workspace, workspace_bytes, adam, stats, s);
    });
}

}  // namespace b747
