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
    const int64_t i = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
    const bool live = i < N;
    const int64_t col = live ? i : N - 1;
    float nv = last_value[col], a = 0.0f;
    int32_t t = T - 1;
    GaeRows<U> cur, nxt;
    gae_load<U>(cur, rew, val, done, t, N, col);
#pragma unroll 1
    for (;;) {
        const int32_t tn = t - U;
        if (tn >= 0) gae_load<U>(nxt, rew, val, done, tn, N, col);
        if (t >= U - 1) gae_steps<U, false>(cur, t, N, col, live, g, gl, nv, a, adv, ret);
        else gae_steps<U, true>(cur, t, N, col, live, g, gl, nv, a, adv, ret);
        if (tn < 0) break;
        cur = nxt;
        t = tn;
    }
}

hipError_t launch_ppo_gae(const float *rew, const float *val, const uint8_t *done, const float *last_value, int32_t T,
                          int64_t N, double gamma, double gae_lambda, float *adv, float *ret, hipStream_t s)
{
    const int64_t blocks = (N + kGaeBlock - 1) / kGaeBlock;
    hipLaunchKernelGGL(k_ppo_gae<kGaeUnroll>, dim3((unsigned)blocks), dim3(kGaeBlock), 0, s, rew, val, done, last_value,
                       T, N, (float)gamma, (float)(gamma * gae_lambda), adv, ret);
    return hipGetLastError();
}

}  // namespace b747
