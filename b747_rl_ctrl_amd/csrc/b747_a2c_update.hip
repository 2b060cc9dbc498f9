// b747_a2c_update.hip -- the fused A2C update (b747_a2c_update.h): its kernels and their launchers, a translation unit
// of their own so that the PPO update's kernels (b747_ppo_update.hip) keep their generated code.
#define B747_POLICY_NO_KERNELS          // PolicyLayout only
#define B747_PPO_UPDATE_PIECES_ONLY     // upd_forward / upd_backward / upd_flush / upd_tiles and the bodies; no PPO kernel
#include "b747_a2c_update.h"

namespace b747 {

// k_ppo_adv_stats for a minibatch whose idx may be NULL (the rows 0 .. batch - 1)
__global__ __launch_bounds__(256) void k_a2c_adv_stats(const float *__restrict__ adv, const int64_t *__restrict__ idx,
                                                       int64_t batch, double *__restrict__ part)
{
    constexpr bool POP = false;
    constexpr int LOSS = kUpdLossA2c;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
#include "b747_ppo_adv_stats_body.h"
}

// k_ppo_grad<OD> with the A2C row (upd_tiles, kUpdLossA2c).  sums (per workgroup, fp64): A logp, (ret - value)^2, 0, 0,
// |A logp|, 0 over the workgroup's rows, then dLoss/d mean, dLoss/d value and dLoss/d log_std summed over them.
// idx NULL: the rows 0 .. batch - 1.  adv_part NULL: A = adv (no normalize_advantage).
template <int OD>
__global__ __launch_bounds__(256) void k_a2c_grad(const float *__restrict__ theta, const float *__restrict__ obs,
                                                  const float *__restrict__ act, const float *__restrict__ adv,
                                                  const float *__restrict__ ret, const int64_t *__restrict__ idx,
                                                  int64_t batch, double vf_coef, const double *__restrict__ adv_part,
                                                  float *__restrict__ gpart, double *__restrict__ spart)
{
    constexpr bool POP = false;
    constexpr int LOSS = kUpdLossA2c;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
    constexpr const float *old_logp = nullptr;   // (the PPO row's: named by the body, read by neither net here)
    constexpr double clip = 0.0;
#include "b747_ppo_grad_body.h"
}

// k_ppo_reduce's text: slot 0 of the sums is A logp, so its statistics row reads [policy loss, value loss, entropy
// loss, 0, 0, mean |A logp|, 0, loss]
__global__ __launch_bounds__(256) void k_a2c_reduce(const float *__restrict__ gpart, const double *__restrict__ spart,
                                                    int n_wg, int n_params, int ba_at, int bv_at, int log_std_at,
                                                    const float *__restrict__ theta, int64_t batch, float ent_coef,
                                                    float vf_coef, float *__restrict__ grad, float *__restrict__ stats)
{
    constexpr bool POP = false;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
#include "b747_ppo_reduce_body.h"
}

// clip_grad_norm_ + RMSprop (not centred, no momentum, no weight decay) on the flat vector, one workgroup as k_ppo_adam:
// g = grad_scale grad, coef = min(1, max_norm / (|g| + 1e-6)), gc = g coef, sq = alpha sq + (1 - alpha) gc^2,
// theta -= lr gc / (sqrt(sq) + eps) (torch.optim.RMSprop) or lr gc / sqrt(sq + eps) (tf_like: SB3's RMSpropTFLike),
// *t += 1.  Element arithmetic in fp64, stored as fp32 (the step reads the stored sq); grad is not written.
__global__ __launch_bounds__(kUpdAdamBlock) void k_ppo_rmsprop(float *__restrict__ theta, float *__restrict__ sq,
                                                               int64_t *__restrict__ t, const float *__restrict__ grad,
                                                               int64_t n, double grad_scale, double max_norm, double lr,
                                                               double alpha, double eps, int tf_like)
{
    __shared__ double red[kUpdAdamBlock];
    const int tid = threadIdx.x;
    double q = 0.0;
    for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
        const double g = (double)(float)(grad_scale * (double)grad[i]);
        q += g * g;
    }
    red[tid] = q;
    __syncthreads();
    for (int w = kUpdAdamBlock / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double norm = sqrt(red[0]);
    const double c0 = max_norm / (norm + 1e-6), coef = c0 < 1.0 ? c0 : 1.0;
    for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
        const double g = (double)(float)((double)(float)(grad_scale * (double)grad[i]) * coef);
        const float sf = (float)(alpha * (double)sq[i] + (1.0 - alpha) * g * g);
        sq[i] = sf;
        const double denom = tf_like ? sqrt((double)sf + eps) : sqrt((double)sf) + eps;
        theta[i] = (float)((double)theta[i] - lr * (g / denom));
    }
    if (tid == 0) t[0] += 1;
}

hipError_t launch_a2c_grad(const float *theta, int od, const UpdData &d, const int64_t *idx, int64_t batch,
                           bool normalize_advantage, double ent_coef, double vf_coef, void *workspace, float *grad,
                           float *stats, hipStream_t s)
{
    return with_obs_dim(od, hipErrorInvalidValue, [&](auto c) {
        constexpr int OD = decltype(c)::value;
        constexpr PolicyLayout L = PolicyLayout::of(OD);
        // the dynamic-LDS limit belongs to the current device's copy of the kernel (a host-side setting, per call)
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_a2c_grad<OD>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, UpdLds<OD>::bytes);
        if (attr != hipSuccess) return attr;
        char *ws = static_cast<char *>(workspace);
        double *adv_part = reinterpret_cast<double *>(ws + upd_ws_adv());
        double *spart = reinterpret_cast<double *>(ws + upd_ws_sums());
        float *gpart = reinterpret_cast<float *>(ws + upd_ws_grad());
        const int n_wg = upd_n_wg(batch);
        if (normalize_advantage)
            hipLaunchKernelGGL(k_a2c_adv_stats, dim3(kUpdAdvBlocks), dim3(256), 0, s, d.adv, idx, batch, adv_part);
        hipLaunchKernelGGL(k_a2c_grad<OD>, dim3(n_wg), dim3(256), UpdLds<OD>::bytes, s, theta, d.obs, d.act, d.adv, d.ret,
                           idx, batch, vf_coef, normalize_advantage ? adv_part : (const double *)nullptr, gpart, spart);
        hipLaunchKernelGGL(k_a2c_reduce, dim3((L.total + 1 + 255) / 256), dim3(256), 0, s, gpart, spart, n_wg, L.total,
                           L.ba, L.bv, L.log_std, theta, batch, (float)ent_coef, (float)vf_coef, grad, stats);
        return hipGetLastError();
    });
}

hipError_t launch_ppo_rmsprop(float *theta, float *sq, int64_t *t, const float *grad, int64_t n_params, double grad_scale,
                              const UpdRms &rms, double lr, hipStream_t s)
{
    hipLaunchKernelGGL(k_ppo_rmsprop, dim3(1), dim3(kUpdAdamBlock), 0, s, theta, sq, t, grad, n_params, grad_scale,
                       rms.max_grad_norm, lr, rms.alpha, rms.eps, rms.tf_like ? 1 : 0);
    return hipGetLastError();
}

}  // namespace b747
