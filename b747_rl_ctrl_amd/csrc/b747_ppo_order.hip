// b747_ppo_order.hip -- one uniformly drawn sample order per population member in one launch (b747_ppo_order.h;
// DESIGN.md 18): the kernel and its launcher, a translation unit of their own so that the kernels of the other units
// keep their generated code.
//
// Member p's local row l = t * envs_per_policy + j gets the 32-bit word u(p, l): word l & 3 of the Philox4x32-10 block
// (Rng::refill's rounds, b747_env.h) with counter (l >> 2, p, lo32(sb), epoch) and key
// K = (seed ^ kOrderTag) ^ ((sb >> 32) * kOrderFold), sb = *step_base read here.  The rows leave in ascending order of
// the 64-bit key (u << 32) | l -- a stable argsort of u, every key distinct, so any correct sort gives this order --
// mapped to the rollout buffers' row numbers t * N + p * envs_per_policy + j.  Integer only.
#include "b747_env.h"   // Rng
#include "b747_ppo_order.h"

namespace b747 {

namespace {

// One compare-exchange of a bitonic network on the element e a lane holds, its partner e ^ j in the same wave
// (j <= 32): the lower element of a pair keeps the smaller key where the run of k elements ascends.
__device__ __forceinline__ uint64_t order_cx(uint64_t v, uint32_t e, uint32_t j, uint32_t k)
{
    const uint64_t o = __shfl_xor((unsigned long long)v, (int)j);
    const bool keep_min = ((e & k) == 0) == ((e & j) == 0);
    return (v < o) == keep_min ? v : o;
}

}  // namespace

// One workgroup = one member.  keys[n_pad] in dynamic LDS, n_pad the next power of two of n_rows (at least 64, at most
// kOrderMaxRows), the tail all-ones: it sorts behind every real key and is never written out.  blockDim.x is a power
// of two, a multiple of 64 and at most n_pad, so whole waves take part in every loop below.
//   * The keys: one Philox block per four rows (n_rows is a multiple of 64: a block is all rows or all padding).
//   * The sort: bitonic.  Runs of k <= 64 and the steps j <= 32 of every longer run stay inside 64 consecutive
//     elements: a wave holds them in registers, one per lane, and exchanges them with cross-lane moves -- no LDS
//     traffic, no barrier between those steps.  The steps j >= 64 go through LDS, one pair per thread and pass, a
//     workgroup barrier after each.
//   * The rows: thread i maps the low word of keys[i] and stores 8 bytes at perm[p][i], consecutive lanes consecutive
//     addresses.
__global__ __launch_bounds__(kOrderMaxBlock) void k_sample_orders(int64_t *__restrict__ perm, uint32_t n_rows,
                                                                  uint32_t n_pad, uint32_t epp, int64_t N,
                                                                  uint64_t seed,
                                                                  const uint64_t *__restrict__ step_base,
                                                                  uint32_t epoch)
{
    extern __shared__ uint64_t order_keys[];
    uint64_t *const keys = order_keys;
    const uint32_t tid = threadIdx.x, nt = blockDim.x, p = blockIdx.x;
    const uint64_t sb = step_base ? *step_base : 0ull;
    const uint64_t key = (seed ^ kOrderTag) ^ ((sb >> 32) * kOrderFold);

    for (uint32_t q = tid; q < n_pad / 4; q += nt) {
        const uint32_t l = 4 * q;
        uint64_t w[4] = {~0ull, ~0ull, ~0ull, ~0ull};
        if (l < n_rows) {
            Rng g;
            g.k0 = (uint32_t)key; g.k1 = (uint32_t)(key >> 32);
            g.c0 = q; g.c1 = p; g.c2 = (uint32_t)sb; g.c3 = epoch;
            g.refill();
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = ((uint64_t)g.buf[i] << 32) | (l + i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) keys[l + i] = w[i];
    }
    __syncthreads();

    // runs of 2 .. 64
    for (uint32_t e = tid; e < n_pad; e += nt) {
        uint64_t v = keys[e];
#pragma unroll
        for (uint32_t k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (uint32_t j = k >> 1; j > 0; j >>= 1) v = order_cx(v, e, j, k);
        keys[e] = v;
    }
    __syncthreads();

    for (uint32_t k = 128; k <= n_pad; k <<= 1) {
        for (uint32_t j = k >> 1; j >= 64; j >>= 1) {
            for (uint32_t i = tid; i < n_pad / 2; i += nt) {
                const uint32_t a = 2 * i - (i & (j - 1)), b = a + j;      // the pair's lower and upper element
                const uint64_t x = keys[a], y = keys[b];
                if ((x > y) == ((a & k) == 0)) {
                    keys[a] = y;
                    keys[b] = x;
                }
            }
            __syncthreads();
        }
        for (uint32_t e = tid; e < n_pad; e += nt) {
            uint64_t v = keys[e];
#pragma unroll
            for (uint32_t j = 32; j > 0; j >>= 1) v = order_cx(v, e, j, k);
            keys[e] = v;
        }
        __syncthreads();
    }

    int64_t *const out = perm + (int64_t)p * n_rows;
    const int64_t col = (int64_t)p * epp;
    for (uint32_t i = tid; i < n_rows; i += nt) {
        const uint32_t l = (uint32_t)keys[i], t = l / epp, j = l - t * epp;
        out[i] = (int64_t)t * N + col + j;
    }
}

hipError_t launch_ppo_sample_orders(int64_t *perm, int32_t n_policies, int32_t T, int32_t envs_per_policy, int64_t N,
                                    uint64_t seed, const uint64_t *step_base, uint32_t epoch, hipStream_t s)
{
    const uint32_t n_rows = (uint32_t)T * (uint32_t)envs_per_policy;
    uint32_t n_pad = 64;
    while (n_pad < n_rows) n_pad <<= 1;
    const size_t lds = (size_t)n_pad * sizeof(uint64_t);
    // above 64 KiB the dynamic-LDS limit has to be raised (a host-side setting of the current device's copy of the
    // kernel, no stream work: b747_ppo_update.hip's grad_lds_limit)
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sample_orders),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(kOrderMaxRows * sizeof(uint64_t)));
        if (e != hipSuccess) return e;
    }
    const uint32_t block = n_pad < (uint32_t)kOrderMaxBlock ? n_pad : (uint32_t)kOrderMaxBlock;
    hipLaunchKernelGGL(k_sample_orders, dim3((unsigned)n_policies), dim3(block), lds, s, perm, n_rows, n_pad,
                       (uint32_t)envs_per_policy, N, seed, step_base, epoch);
    return hipGetLastError();
}

}  // namespace b747
