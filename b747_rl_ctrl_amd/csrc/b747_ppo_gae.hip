// b747_ppo_gae.hip -- generalized advantage estimation over a time-major rollout in one launch (b747_ppo_gae.h): the
// kernel and its launcher, a translation unit of their own so that the kernels of the other units keep their
// generated code.
//
// PPO.compute_gae's torch loop (SB3 1.4 RolloutBuffer.compute_returns_and_advantage), one fp32 rounding per operation
// in torch's order: per env a = 0, and for t = T-1 .. 0
//   nv = t == T-1 ? last_value : val[t+1];   nt = done[t] ? 0 : 1;
//   delta = (rew[t] + (g nv) nt) - val[t];   a = delta + (gl nt) a;   adv[t] = a;   ret[t] = a + val[t]
// with g = (float)gamma and gl = (float)(gamma gae_lambda), the double product rounded once.  The multiply by nt
// stays a multiply (torch's operation sequence, non-finite values included) and nothing contracts into an FMA (the
// build's -ffp-contract=off, repeated below): the results are torch's bit for bit (tests/test_gpu_ppo_gae.py).
#include "../../include/b747.h"   // the hyper-parameter table's layout (B747_PPO_HYPER_*)
#include "b747_ppo_gae.h"

#pragma clang fp contract(off)

namespace b747 {

namespace {

// The rows t, t-1, .. t-U+1 of one env (rows below 0 repeat row 0: a valid address, never used)
template <int U>
struct GaeRows {
    float r[U], v[U];
    uint8_t d[U];
};

template <int U>
__device__ __forceinline__ void gae_load(GaeRows<U> &x, const float *__restrict__ rew, const float *__restrict__ val,
                                         const uint8_t *__restrict__ done, int32_t t, int64_t N, int64_t col)
{
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int32_t tt = t - k > 0 ? t - k : 0;
        const int64_t row = (int64_t)tt * N + col;
        x.r[k] = rew[row];
        x.v[k] = val[row];
        x.d[k] = done[row];
    }
}

// The recurrence over the chunk's rows (PART: those at or above row 0 only).  nv enters as the value of row t + 1 and
// leaves as that of the chunk's last row: each step's val load is the next step's nv.
template <int U, bool PART>
__device__ __forceinline__ void gae_steps(const GaeRows<U> &x, int32_t t, int64_t N, int64_t col, bool live, float g,
                                          float gl, float &nv, float &a, float *__restrict__ adv, float *__restrict__ ret)
{
#pragma unroll
    for (int k = 0; k < U; ++k) {
        if (PART && t - k < 0) break;               // (wave-uniform)
        const float nt = x.d[k] ? 0.0f : 1.0f;
        const float delta = (x.r[k] + ((g * nv) * nt)) - x.v[k];
        a = delta + ((gl * nt) * a);
        if (live) {
            const int64_t row = (int64_t)(t - k) * N + col;
            adv[row] = a;
            ret[row] = a + x.v[k];
        }
        nv = x.v[k];
    }
}

}  // namespace

// One lane per env, the time loop backwards in chunks of U rows.  A step's loads do not depend on the recurrence:
// the next chunk's 3 U loads are issued before the current chunk's arithmetic, so a small batch pays one exposed
// load latency per U steps, not one per step.  Lanes past N read env N - 1's rows and store nothing.
// adv / ret must not alias the inputs.
template <int U>
__global__ __launch_bounds__(kGaeBlock) void k_ppo_gae(const float *__restrict__ rew, const float *__restrict__ val,
                                                       const uint8_t *__restrict__ done,
                                                       const float *__restrict__ last_value, int32_t T, int64_t N,
                                                       float g, float gl, float *__restrict__ adv,
                                                       float *__restrict__ ret)
{
#include "b747_ppo_gae_body.h"
}

// k_ppo_gae<U> for a population (b747_ppo_gae_population): env i belongs to member i / envs_per_policy
// and takes g and gl from that member's row of the hyper-parameter table.  envs_per_policy is a multiple of kGaeBlock
// (groups = envs_per_policy / kGaeBlock workgroups per member), so the member is uniform over the workgroup and its two
// doubles are loaded once, here; the product is fp64, rounded once -- launch_ppo_gae's rounding on the host.  A lane
// past N copies env N - 1: the same wave, so the same member.
template <int U>
__global__ __launch_bounds__(kGaeBlock) void k_pop_gae(const float *__restrict__ rew, const float *__restrict__ val,
                                                       const uint8_t *__restrict__ done,
                                                       const float *__restrict__ last_value, int32_t T, int64_t N,
                                                       uint32_t groups, const double *__restrict__ hyper,
                                                       float *__restrict__ adv, float *__restrict__ ret)
{
    const double *row = hyper + (int64_t)(blockIdx.x / groups) * B747_PPO_HYPER_COLS;
    const double gamma = row[B747_PPO_HYPER_GAMMA], gae_lambda = row[B747_PPO_HYPER_GAE_LAMBDA];
    const float g = (float)gamma, gl = (float)(gamma * gae_lambda);
#include "b747_ppo_gae_body.h"
}

hipError_t launch_ppo_gae(const float *rew, const float *val, const uint8_t *done, const float *last_value, int32_t T,
                          int64_t N, double gamma, double gae_lambda, float *adv, float *ret, hipStream_t s)
{
    const int64_t blocks = (N + kGaeBlock - 1) / kGaeBlock;
    hipLaunchKernelGGL(k_ppo_gae<kGaeUnroll>, dim3((unsigned)blocks), dim3(kGaeBlock), 0, s, rew, val, done, last_value,
                       T, N, (float)gamma, (float)(gamma * gae_lambda), adv, ret);
    return hipGetLastError();
}

hipError_t launch_ppo_gae_population(const float *rew, const float *val, const uint8_t *done, const float *last_value,
                                     int32_t T, int64_t N, int32_t envs_per_policy, const double *hyper_dev, float *adv,
                                     float *ret, hipStream_t s)
{
    // a workgroup must lie inside one member (envs_per_policy is a multiple of 64): a build with another block size
    // (-DB747_GAE_BLOCK, an experiment's) has no population kernel, and says so
    if (kGaeBlock != 64) return hipErrorInvalidDeviceFunction;
    const int64_t blocks = (N + kGaeBlock - 1) / kGaeBlock;
    hipLaunchKernelGGL(k_pop_gae<kGaeUnroll>, dim3((unsigned)blocks), dim3(kGaeBlock), 0, s, rew, val, done, last_value,
                       T, N, (uint32_t)(envs_per_policy / kGaeBlock), hyper_dev, adv, ret);
    return hipGetLastError();
}

}  // namespace b747
