// b747_a2c_population.hip -- the member-batched A2C update (b747_a2c_population.h): its kernels and their launcher, a
// translation unit of their own so that the kernels of b747_ppo_update.hip and b747_a2c_update.hip keep their
// generated code.
#define B747_POLICY_NO_KERNELS          // PolicyLayout only
#define B747_PPO_UPDATE_PIECES_ONLY     // upd_forward / upd_backward / upd_flush / upd_tiles and the bodies; no PPO kernel
#include "b747_a2c_population.h"

namespace b747 {

// k_a2c_adv_stats for every member of a chunk: grid (kUpdAdvBlocks, members).  idx (the index table's row) and part
// are member 0's.
__global__ __launch_bounds__(256) void k_apop_adv_stats(const float *__restrict__ adv, const int64_t *__restrict__ idx,
                                                        int64_t batch, double *__restrict__ part, UpdPopArgs pa)
{
    constexpr bool POP = true;
    constexpr int LOSS = kUpdLossA2c;
#include "b747_ppo_adv_stats_body.h"
}

// k_a2c_grad<OD> for every member of a chunk: grid (n_wg, members), n_wg what the member's own launch has.  theta, idx
// and the three workspace pointers are member 0's; the member's vf_coef comes from its row of the table (hyper_dev is
// member 0's row), a workgroup-uniform load as k_hyp_grad's.  adv_part NULL: no normalize_advantage.
template <int OD>
__global__ __launch_bounds__(256) void k_apop_grad(const float *__restrict__ theta, const float *__restrict__ obs,
                                                   const float *__restrict__ act, const float *__restrict__ adv,
                                                   const float *__restrict__ ret, const int64_t *__restrict__ idx,
                                                   int64_t batch, const double *__restrict__ hyper_dev,
                                                   const double *__restrict__ adv_part, float *__restrict__ gpart,
                                                   double *__restrict__ spart, UpdPopArgs pa)
{
    constexpr bool POP = true;
    constexpr int LOSS = kUpdLossA2c;
    const double vf_coef = hyper_dev[(int64_t)blockIdx.y * B747_PPO_HYPER_COLS + B747_PPO_HYPER_VF_COEF];
    constexpr const float *old_logp = nullptr;   // (the PPO row's: named by the body, read by neither net here)
    constexpr double clip = 0.0;
#include "b747_ppo_grad_body.h"
}

// k_a2c_reduce for every member of a chunk, the member's ent_coef and vf_coef from the table, rounded to float here
// (the launcher's rounding of k_a2c_reduce's arguments)
__global__ __launch_bounds__(256) void k_apop_reduce(const float *__restrict__ gpart, const double *__restrict__ spart,
                                                     int n_wg, int n_params, int ba_at, int bv_at, int log_std_at,
                                                     const float *__restrict__ theta, int64_t batch,
                                                     const double *__restrict__ hyper_dev, float *__restrict__ grad,
                                                     float *__restrict__ stats, UpdPopArgs pa)
{
    constexpr bool POP = true;
    const double *hyp = hyper_dev + (int64_t)blockIdx.y * B747_PPO_HYPER_COLS;
    const float ent_coef = (float)hyp[B747_PPO_HYPER_ENT_COEF], vf_coef = (float)hyp[B747_PPO_HYPER_VF_COEF];
#include "b747_ppo_reduce_body.h"
}

// clip_grad_norm_ and the member's optimiser for every member of a chunk: grid (1, members), one workgroup per member.
// theta, state0, state1, t, grad (in the workspace) and hyper_dev are member 0's.  The member's max_norm, lr and kind
// come from its table row; the kind (B747_OPT_RMSPROP, B747_OPT_RMSPROP_TF, anything else: Adam) is the same for the
// whole workgroup, so the branch on it does not diverge.  The norm and the clipped gradient are k_ppo_rmsprop's and
// k_ppo_adam's with grad_scale 1 (1.0 * g rounded to float is g).  RMSprop: k_ppo_rmsprop's element arithmetic on
// state0 = sq.  Adam: b747_ppo_adam_body.h's on state0 = m, state1 = v.  fp64 element arithmetic, fp32 stores, the
// steps read the stored values; the step count moves by one for every kind.
// The two pow of Adam's bias corrections keep their many fp64 constants in SGPR pairs.  They are therefore
// evaluated first, one after the other (the scheduling barrier keeps the two chains apart), while little else is live:
// the vector length is pa.n_params, not an argument of its own, and the member's max_norm and lr are loaded after the
// norm's reduction.  With that the kernel spills no SGPR (tests/test_a2c_population_resources.py); the order of
// evaluation changes no operation.
__global__ __launch_bounds__(kUpdAdamBlock) void k_apop_opt(float *__restrict__ theta, float *__restrict__ state0,
                                                            float *__restrict__ state1, int64_t *__restrict__ t,
                                                            const float *__restrict__ grad,
                                                            const double *__restrict__ hyper_dev, double alpha,
                                                            double rms_eps, double beta1, double beta2, double adam_eps,
                                                            UpdPopArgs pa)
{
    const double *hyp = hyper_dev + (int64_t)blockIdx.y * B747_PPO_HYPER_COLS;
    const double kind = hyp[B747_PPO_HYPER_OPTIMIZER];
    const bool tf_like = kind == (double)B747_OPT_RMSPROP_TF, rms = tf_like || kind == (double)B747_OPT_RMSPROP;
    theta += (int64_t)blockIdx.y * pa.policy_stride;
    state0 += (int64_t)blockIdx.y * pa.n_params;
    state1 += (int64_t)blockIdx.y * pa.n_params;
    t += blockIdx.y;
    grad = reinterpret_cast<const float *>(reinterpret_cast<const char *>(grad) + (int64_t)blockIdx.y * pa.ws_stride);
    const int64_t n = pa.n_params;
    __shared__ double red[kUpdAdamBlock];
    const int tid = threadIdx.x;
    const int64_t step = t[0] + 1;
    double bc1 = 1.0, bc2s = 1.0;
    if (!rms) {
        bc1 = 1.0 - pow(beta1, (double)step);
        __builtin_amdgcn_sched_barrier(0);
        bc2s = sqrt(1.0 - pow(beta2, (double)step));
    }
    double q = 0.0;
    for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
        const double g = (double)grad[i];
        q += g * g;
    }
    red[tid] = q;
    __syncthreads();
    for (int w = kUpdAdamBlock / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double max_norm = hyp[B747_PPO_HYPER_MAX_GRAD_NORM], lr = hyp[B747_PPO_HYPER_LR];
    const double norm = sqrt(red[0]);
    const double c0 = max_norm / (norm + 1e-6), coef = c0 < 1.0 ? c0 : 1.0;
    if (rms) {
        for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
            const double g = (double)(float)((double)grad[i] * coef);
            const float sf = (float)(alpha * (double)state0[i] + (1.0 - alpha) * g * g);
            state0[i] = sf;
            const double denom = tf_like ? sqrt((double)sf + rms_eps) : sqrt((double)sf) + rms_eps;
            theta[i] = (float)((double)theta[i] - lr * (g / denom));
        }
    } else {
        const double step_size = lr / bc1;
        for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
            const double g = (double)(float)((double)grad[i] * coef);
            const double mi = (double)state0[i] + (1.0 - beta1) * (g - (double)state0[i]);
            const double vi = beta2 * (double)state1[i] + (1.0 - beta2) * g * g;
            const float mf = (float)mi, vf = (float)vi;
            state0[i] = mf;
            state1[i] = vf;
            theta[i] = (float)((double)theta[i] - step_size * ((double)mf / (sqrt((double)vf) / bc2s + adam_eps)));
        }
    }
    if (tid == 0) t[0] = step;   // (every thread read the old count before the first barrier)
}

hipError_t launch_a2c_update_population(const UpdPopState &st, int n_policies, int64_t policy_stride, int od,
                                        const UpdData &d, const int64_t *rows, int64_t rows_stride, int64_t batch,
                                        bool normalize_advantage, const double *hyper_dev, void *workspace,
                                        int64_t workspace_bytes, const UpdPopOpt &opt, float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto c) {
        constexpr int OD = decltype(c)::value;
        constexpr PolicyLayout L = PolicyLayout::of(OD);
        constexpr int P = L.total;
        // the dynamic-LDS limit belongs to the current device's copy of the kernel (a host-side setting, per call)
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_apop_grad<OD>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, UpdLds<OD>::bytes);
        if (attr != hipSuccess) return attr;
        const int64_t per = upd_pop_ws_bytes(OD, batch);
        int64_t chunk = workspace_bytes / per;
        if (chunk > n_policies) chunk = n_policies;
        if (chunk > kUpdPopMaxMembers) chunk = kUpdPopMaxMembers;
        // (n_rows: the distance between two members' rows of the index table)
        const UpdPopArgs pa{policy_stride, P, rows_stride, per, kUpdStats};
        char *ws = static_cast<char *>(workspace);
        double *adv_part = reinterpret_cast<double *>(ws + upd_ws_adv());
        double *spart = reinterpret_cast<double *>(ws + upd_ws_sums());
        float *gpart = reinterpret_cast<float *>(ws + upd_pop_ws_grad(batch));
        float *grad = reinterpret_cast<float *>(ws + upd_pop_ws_out(OD, batch));
        const int n_wg = upd_n_wg(batch);
        for (int64_t c0 = 0; c0 < n_policies; c0 += chunk) {
            const unsigned members = (unsigned)(n_policies - c0 < chunk ? n_policies - c0 : chunk);
            float *th = st.theta + c0 * policy_stride, *row = stats + c0 * kUpdStats;
            const int64_t *idx = rows + c0 * rows_stride;
            const double *hyp = hyper_dev + c0 * B747_PPO_HYPER_COLS;
            if (normalize_advantage)
                hipLaunchKernelGGL(k_apop_adv_stats, dim3(kUpdAdvBlocks, members), dim3(256), 0, s, d.adv, idx, batch,
                                   adv_part, pa);
            hipLaunchKernelGGL(k_apop_grad<OD>, dim3(n_wg, members), dim3(256), UpdLds<OD>::bytes, s, th, d.obs, d.act,
                               d.adv, d.ret, idx, batch, hyp, normalize_advantage ? adv_part : (const double *)nullptr,
                               gpart, spart, pa);
            hipLaunchKernelGGL(k_apop_reduce, dim3((P + 1 + 255) / 256, members), dim3(256), 0, s, gpart, spart, n_wg, P,
                               L.ba, L.bv, L.log_std, th, batch, hyp, grad, row, pa);
            hipLaunchKernelGGL(k_apop_opt, dim3(1, members), dim3(kUpdAdamBlock), 0, s, th, st.state0 + c0 * P,
                               st.state1 + c0 * P, st.t + c0, grad, hyp, opt.rms_alpha, opt.rms_eps,
                               opt.adam_beta1, opt.adam_beta2, opt.adam_eps, pa);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

}  // namespace b747
